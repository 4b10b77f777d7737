"""The scene partition's rule (include/gsr_chunker.h) restated literally per chunk in numpy.

Deliberately the other formulation from csrc/chunker.hip's single pass: a loop over the cells that
tests every point and every camera against that cell's own boxes, a dense id -> position array
(points3d_ordered) for the cameras' visible points, a dict for the observation filter, a boolean
valid-camera array and Python's random for the draws.  Written from the rule, not from the reference
script, which cannot be run beside this project."""
from __future__ import annotations

import random

import numpy as np

IN, NEAR, DRAW = 1, 2, 3
NOT_IN_C = -2
FAR = 1e12


def boxes(bbox, cs, i, j, n_w, n_h):
    """(lo, hi), (plo, phi), (elo, ehi) of cell (i, j): box, pbox and ebox, fp64."""
    x0, y0, cs = float(bbox[0][0]), float(bbox[0][1]), float(cs)
    lo = np.array([x0 + float(i) * cs, y0 + float(j) * cs, -FAR], dtype=np.float64)
    hi = np.array([x0 + float(i + 1) * cs, y0 + float(j + 1) * cs, FAR], dtype=np.float64)
    plo, phi = lo.copy(), hi.copy()
    if i == 0:
        plo[0] = -FAR
    if j == 0:
        plo[1] = -FAR
    if i == n_w - 1:
        phi[0] = FAR
    if j == n_h - 1:
        phi[1] = FAR
    c = (lo + hi) / 2
    h = (hi - lo) / 2
    return (lo, hi), (plo, phi), (c - 2 * h, c + 2 * h)


def inside(p, lo, hi):
    """Strict on every axis; NaN fails.  p: (..., 3) of any float type, compared in fp64."""
    p = np.asarray(p).astype(np.float64)
    if p.size == 0:
        return np.zeros(p.shape[:-1], dtype=bool)
    with np.errstate(invalid="ignore"):
        return np.all(p < hi, axis=-1) & np.all(p > lo, axis=-1)


def partition(cam_centers, obs_ptr, obs_point_id, point_id, point_xyz, point_error, depth_centers, grid, chunk_size,
              min_n_cams=5, max_n_cams=1500, add_far_cams=True, rng=None):
    """Everything gs_train.chunker.partition_scene returns, as numpy: a dict with cell32, cell64,
    memberships32 / memberships64 (in how many cells' pbox each row was found), n_pts, blend, total,
    candidates (K, 5), draws (what the generator returned, in order), chunks (list of dicts) and
    excluded."""
    rng = random.Random(0) if rng is None else rng
    bbox, n_w, n_h = grid
    cam = np.asarray(cam_centers, dtype=np.float32).reshape(-1, 3)
    obs_ptr = np.asarray(obs_ptr, dtype=np.int64)
    obs = np.asarray(obs_point_id, dtype=np.int64)
    ids = np.asarray(point_id, dtype=np.int64)
    xyz64 = np.asarray(point_xyz, dtype=np.float64).reshape(-1, 3)
    err = np.asarray(point_error, dtype=np.float32)
    depth = np.zeros((0, 3)) if depth_centers is None else np.asarray(depth_centers, dtype=np.float64).reshape(-1, 3)
    M, N, cells = len(cam), len(ids), n_w * n_h

    with np.errstate(invalid="ignore"):
        maskC = err < np.float32(10)
    rowsC = np.nonzero(maskC)[0]
    with np.errstate(over="ignore", invalid="ignore"):
        xyzsC = xyz64.astype(np.float32)[maskC]
    indicesC = ids[maskC]
    L = int(indicesC.max()) + 1 if len(indicesC) else 0
    points3d_ordered = np.zeros([L, 3])
    points3d_ordered[indicesC] = xyzsC
    points3d = {int(k): xyz64[r] for r, k in enumerate(ids)}

    images_points3d = []
    for m in range(M):
        pts_idx = obs[obs_ptr[m]:obs_ptr[m + 1]]
        mask = (pts_idx >= 0) & (pts_idx < L)
        pts_idx = pts_idx[mask]
        image_points3d = points3d_ordered[pts_idx] if len(pts_idx) else np.zeros((0, 3))
        nonzero = (image_points3d != 0).sum(axis=-1)
        images_points3d.append(image_points3d[nonzero > 0])

    img_points = np.concatenate(images_points3d + [np.zeros((0, 3))])
    img_owner = np.repeat(np.arange(M), [len(p) for p in images_points3d])
    obs_owner = np.repeat(np.arange(M), np.diff(obs_ptr))
    cell32 = np.where(maskC, -1, NOT_IN_C).astype(np.int32)
    cell64 = np.full(N, -1, dtype=np.int32)
    member32, member64 = np.zeros(N, np.int64), np.zeros(N, np.int64)
    n_pts, blend = np.zeros((M, cells), np.int32), np.zeros((M, cells), np.int32)
    total = np.array([len(p) for p in images_points3d], dtype=np.int32)
    candidates, draws, chunks, excluded = [], [], [], []

    for i in range(n_w):
        for j in range(n_h):
            cell = i * n_h + j
            (lo, hi), (plo, phi), (elo, ehi) = boxes(bbox, chunk_size, i, j, n_w, n_h)
            mask = inside(xyzsC, plo, phi)
            colmap_rows = rowsC[mask]
            colmap_indices = indicesC[mask]
            cell32[colmap_rows] = cell
            member32[colmap_rows] += 1
            in64 = inside(xyz64, plo, phi)
            cell64[in64] = cell
            member64[in64] += 1

            # every camera against this cell: its visible points in pbox, its observations of the cell's
            # points (np.isin), its centre in box and in ebox
            n_pts[:, cell] = np.bincount(img_owner[inside(img_points, plo, phi)], minlength=M)
            blend[:, cell] = np.bincount(obs_owner[np.isin(obs, colmap_indices)], minlength=M)
            in_box, in_ebox = inside(cam, lo, hi), inside(cam, elo, ehi)
            valid_cam = np.zeros(M, dtype=bool)
            for m in np.nonzero(in_box | (n_pts[:, cell] > 10))[0]:
                n = int(n_pts[m, cell])
                state = 0
                if in_box[m]:
                    state = IN
                elif in_ebox[m] and n > 20:
                    state = NEAR
                elif n > 10 and add_far_cams:
                    state = DRAW
                if state:
                    candidates.append((cell, m, state, n, int(total[m])))
                if state == DRAW:
                    u = rng.uniform(0, 0.5)
                    draws.append(("uniform", cell, int(m), u))
                    valid_cam[m] = u < float(n) / len(images_points3d[m])
                elif state:
                    valid_cam[m] = True
            if valid_cam.sum() > max_n_cams:
                for _ in range(int(valid_cam.sum()) - max_n_cams):
                    remove_idx = rng.randint(0, int(valid_cam.sum()) - 1)
                    remove_glob = np.arange(M)[valid_cam][remove_idx]
                    draws.append(("randint", cell, int(remove_glob), remove_idx))
                    valid_cam[remove_glob] = False
            if not valid_cam.sum() > min_n_cams:
                excluded.append((i, j))
                continue
            cameras = np.nonzero(valid_cam)[0].astype(np.int64)
            kept = []
            for m in cameras:
                keep = []
                for o in range(int(obs_ptr[m]), int(obs_ptr[m + 1])):
                    q = int(obs[o])
                    if q >= 0 and q in points3d and bool(inside(points3d[q], plo, phi)):
                        keep.append(o)
                kept.append(np.array(keep, dtype=np.int64))
            chunks.append(dict(i=i, j=j, cell=cell, center=(lo + hi) / 2, extent=hi - lo, cameras=cameras, obs=kept,
                               points=colmap_rows.astype(np.int64), blend=blend[cameras, cell].copy(),
                               depth_cameras=np.nonzero(inside(depth, lo, hi))[0].astype(np.int64)))
    cand = np.array(candidates, dtype=np.int32).reshape(-1, 5)
    return dict(cell32=cell32, cell64=cell64, memberships32=member32, memberships64=member64, n_pts=n_pts, blend=blend,
                total=total, candidates=cand, draws=draws, chunks=chunks, excluded=excluded)
