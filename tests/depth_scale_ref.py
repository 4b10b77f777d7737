"""The depth scale fit in numpy (include/gsr_depth_scale.h's rule), for one image.

fit_image   the rule as the project states it: fp64 where it says fp64, fp32 where it says fp32, the two
            sums of absolute deviations formed exactly (math.fsum) and rounded once.
literal     preprocess/make_depth_scale.py:19-75 line by line, with numpy's own median and mean (its
            float32 pairwise mean of s_mono included) and `sample` in the place of cv2.remap.
Both return None for an image without a map, else a dict.  fit_image takes `mutant` to break one part of
the rule on purpose (tests/test_depth_scale_cpu.py checks that the cases notice each)."""
from __future__ import annotations

import math

import numpy as np

MUTANTS = ("ge_10", "range_over_valid", "round_half_up", "no_clamp", "upper_median", "bound_fp64", "missing_swapped")


def qvec2rotmat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def sample(src, mx, my, mutant=None):
    """The bilinear sample of src (Hd, Wd) float32 at (mx, my) float32 arrays: (n,) float32."""
    src = np.asarray(src, np.float32)
    Hd, Wd = src.shape
    mx, my = np.asarray(mx, np.float32), np.asarray(my, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        px, py = mx * np.float32(32), my * np.float32(32)
        if mutant == "round_half_up":
            fsx, fsy = np.floor(px + np.float32(0.5)), np.floor(py + np.float32(0.5))
        else:
            fsx, fsy = np.rint(px), np.rint(py)
        sx = np.minimum(fsx, np.float32(2.0 ** 30)).astype(np.int64)
        sy = np.minimum(fsy, np.float32(2.0 ** 30)).astype(np.int64)
    ix, iy = sx >> 5, sy >> 5
    fx, fy = (sx & 31).astype(np.float32) / np.float32(32), (sy & 31).astype(np.float32) / np.float32(32)
    if mutant == "no_clamp":  # wrap instead of replicating the border
        x0, x1, y0, y1 = ix % Wd, (ix + 1) % Wd, iy % Hd, (iy + 1) % Hd
    else:
        x0, x1 = np.clip(ix, 0, Wd - 1), np.clip(ix + 1, 0, Wd - 1)
        y0, y1 = np.clip(iy, 0, Hd - 1), np.clip(iy + 1, 0, Hd - 1)
    one = np.float32(1)
    w00, w01, w10, w11 = (one - fy) * (one - fx), (one - fy) * fx, fy * (one - fx), fy * fx
    v = ((src[y0, x0] * w00 + src[y0, x1] * w01) + src[y1, x0] * w10) + src[y1, x1] * w11
    return v.astype(np.float32)


def _median(a):
    """Sorted middle, or fl(a + b) / 2 of the two middle values, in a's dtype."""
    s = np.sort(a)
    n = len(s)
    if n & 1:
        return s[n // 2]
    return (s[n // 2 - 1] + s[n // 2]) / s.dtype.type(2)


def fit_image(q, t, width, height, xy, pid, point_id, point_xyz, u16, missing="origin", mutant=None):
    if u16 is None:
        return None
    if mutant == "missing_swapped":
        missing = "skip" if missing == "origin" else "origin"
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    xy, pid = np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(pid, np.int64)
    point_id, point_xyz = np.asarray(point_id, np.int64), np.asarray(point_xyz, np.float64).reshape(-1, 3)
    u16 = np.asarray(u16)
    Hd, Wd = u16.shape
    T = int(point_id.max()) + 1 if len(point_id) else 0
    table = np.full(T, -1, np.int64)
    table[point_id] = np.arange(len(point_id))
    masked = (pid >= 0) & (pid < T)
    row = np.where(masked, table[np.where(masked, pid, 0)] if T else -1, -1)
    if missing == "skip":
        masked &= row >= 0
    P = np.where((row >= 0)[:, None], point_xyz[np.maximum(row, 0)] if len(point_xyz) else 0.0, 0.0)
    R = qvec2rotmat(q)
    with np.errstate(all="ignore"):
        z = ((R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1]) + R[2, 2] * P[:, 2]) + t[2]
        inv = 1.0 / z
        s = float(Hd) / float(height)
        m = (xy * s).astype(np.float32)
        if mutant == "bound_fp64":
            bw, bh = float(width) * s, float(height) * s
            valid = masked & (m[:, 0] >= 0) & (m[:, 1] >= 0) & (m[:, 0].astype(np.float64) < bw) & \
                (m[:, 1].astype(np.float64) < bh) & (inv > 0)
        else:
            bw, bh = np.float32(float(width) * s), np.float32(float(height) * s)
            valid = masked & (m[:, 0] >= 0) & (m[:, 1] >= 0) & (m[:, 0] < bw) & (m[:, 1] < bh) & (inv > 0)
        n_valid = int(valid.sum())
        over = inv[valid] if mutant == "range_over_valid" else inv[masked]
        nan_seen = bool(np.isnan(inv[masked]).any())
        wide = bool(len(over) and (over.max() - over.min()) > 1e-3)
    out = dict(scale=0.0, offset=0.0, t_colmap=0.0, s_colmap=0.0, t_mono=0.0, s_mono=0.0, n_valid=n_valid, fitted=False,
               nan_seen=nan_seen)
    enough = n_valid >= 10 if mutant == "ge_10" else n_valid > 10
    if not (enough and wide) or n_valid == 0:
        return out
    iv = inv[valid]
    src = u16.astype(np.float32) / np.float32(65536)
    v = sample(src, m[valid, 0], m[valid, 1], mutant)
    if mutant == "upper_median":
        t_colmap, t_mono = np.sort(iv)[n_valid // 2], np.sort(v)[n_valid // 2]
    else:
        t_colmap, t_mono = _median(iv), _median(v)
    with np.errstate(all="ignore"):
        s_colmap = np.float64(math.fsum(np.abs(iv - t_colmap).tolist())) / np.float64(n_valid)
        s_mono = np.float64(math.fsum(np.abs(v - t_mono).astype(np.float32).astype(np.float64).tolist())) / \
            np.float64(n_valid)
        scale = np.float64(s_colmap) / np.float64(s_mono)
        offset = np.float64(t_colmap) - np.float64(t_mono) * scale
    out.update(scale=float(scale), offset=float(offset), t_colmap=float(t_colmap), s_colmap=float(s_colmap),
               t_mono=float(t_mono), s_mono=float(s_mono), fitted=True)
    return out


def literal(q, t, width, height, xy, pid, point_id, point_xyz, u16, ordered=None):
    """make_depth_scale.py:19-75 with its own names; also returns the four statistics.  ordered: the
    script's points3d_ordered (:87-90), which it builds once for all images; built here when not given."""
    if u16 is None:
        return None
    points3d_ordered = ordered
    if points3d_ordered is None:
        pts_indices, pts_xyzs = np.asarray(point_id, np.int64), np.asarray(point_xyz, np.float64).reshape(-1, 3)
        points3d_ordered = np.zeros([pts_indices.max() + 1, 3])
        points3d_ordered[pts_indices] = pts_xyzs
    pts_idx = np.asarray(pid, np.int64)
    mask = pts_idx >= 0
    mask *= pts_idx < len(points3d_ordered)
    pts_idx = pts_idx[mask]
    valid_xys = np.asarray(xy, np.float64).reshape(-1, 2)[mask]
    if len(pts_idx) > 0:
        pts = points3d_ordered[pts_idx]
    else:
        pts = np.array([0, 0, 0])
    R = qvec2rotmat(np.asarray(q, np.float64))
    with np.errstate(all="ignore"):
        pts = np.dot(pts, R.T) + np.asarray(t, np.float64)
        invcolmapdepth = 1. / pts[..., 2]
        invmonodepthmap = np.asarray(u16).astype(np.float32) / (2 ** 16)
        s = invmonodepthmap.shape[0] / height
        maps = (valid_xys * s).astype(np.float32)
        valid = ((maps[..., 0] >= 0) * (maps[..., 1] >= 0) * (maps[..., 0] < width * s) * (maps[..., 1] < height * s)
                 * (invcolmapdepth > 0))
        out = dict(scale=0, offset=0, t_colmap=0.0, s_colmap=0.0, t_mono=0.0, s_mono=0.0, n_valid=int(valid.sum()))
        if valid.sum() > 10 and (invcolmapdepth.max() - invcolmapdepth.min()) > 1e-3:
            maps = maps[valid, :]
            invcolmapdepth = invcolmapdepth[valid]
            invmonodepth = sample(invmonodepthmap, maps[..., 0], maps[..., 1])
            t_colmap = np.median(invcolmapdepth)
            s_colmap = np.mean(np.abs(invcolmapdepth - t_colmap))
            t_mono = np.median(invmonodepth)
            s_mono = np.mean(np.abs(invmonodepth - t_mono))
            scale = s_colmap / s_mono
            offset = t_colmap - t_mono * scale
            out.update(scale=float(scale), offset=float(offset), t_colmap=float(t_colmap), s_colmap=float(s_colmap),
                       t_mono=float(t_mono), s_mono=float(s_mono))
    return out
