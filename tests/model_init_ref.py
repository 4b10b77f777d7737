"""numpy reference of the model construction from a cloud and of the scaffold selection:
scene/gaussian_model.py:163-264 (create_from_pcd) restated for tests/test_model_init_cpu.py and
tests/test_gpu_model_init.py.  Importable without a GPU and without torch.

What the reference decides or copies in float32 is float32 here, to the bit:

    min, max, mean = 0.5 * (min + max)                         :178-180
    the cloud rows' xyz and colour, rotation (1, 0, 0, 0)      :197-198, :212-213
    SH DC = (rgb - 0.5) / float32(0.28209479177387814)         :204 (RGB2SH: a division)
    d = max(dist2, 1e-7); skybox mode: d * 10 on the skybox rows, min(d, 10) on the others  :207-210
    the raw 0.7 of the skybox rows' opacity                    :217
    selec = m > 0.5 * e0 and m < float32(1.5 * e0), m = max(|x - cx|, |y - cy|) with torch.max's
            NaN (either side NaN -> NaN -> not selected); rows below skybox_points always  :248-252

What goes through a transcendental function is float64 here, from the float32 inputs, and the
kernel's float32 value is compared with it within a derived bound:

    radius = ||max - mean||                                    :188
    theta = 2 pi u_theta, cos(phi) = 1 - 1.4 u_phi, sin(phi) = sqrt(1 - cos(phi)^2)
    skybox xyz = mean + 10 radius (cos theta sin phi, sin theta sin phi, cos phi)   :190-196
    scaling = log(sqrt(d))                                     :211
    opacity = log(x / (1 - x)), x = 0.02 (skybox mode) or 0.01 :216, :219

dist2 is simple_knn's distCUDA2; knn_mean_dist2 below is the brute-force restatement with
include/gsr_knn.h's summation order (the C oracle's gso_knn_mean_dist2 is the bit-exact one; this
one emulates the fp32 fma in float64, which rounds twice in rare cases).
"""
from __future__ import annotations

import numpy as np

C0 = np.float32(0.28209479177387814)  # utils/sh_utils.py:26, as torch rounds the scalar
SKY_RGB = np.array([0.7, 0.8, 0.95], np.float32)  # ones * 0.7 / 0.8 / 0.95 in float32 (:198-201)
F32 = np.float32


def logit(x: float) -> float:
    return float(np.log(x / (1.0 - x)))


def knn_mean_dist2(points) -> np.ndarray:
    """(d0 + d1 + d2) / 3 over the three nearest other points (by index), float32; FLT_MAX for the
    missing neighbours of N < 4.  d = fma(dz, dz, fma(dy, dy, dx * dx))."""
    p = np.asarray(points, F32)
    N = p.shape[0]
    out = np.empty(N, F32)
    big = np.finfo(F32).max
    for i in range(N):
        d = (p - p[i]).astype(F32)
        a = (d[:, 0] * d[:, 0]).astype(F32)
        a = (d[:, 1].astype(np.float64) * d[:, 1].astype(np.float64) + a.astype(np.float64)).astype(F32)
        a = (d[:, 2].astype(np.float64) * d[:, 2].astype(np.float64) + a.astype(np.float64)).astype(F32)
        a = np.delete(a, i)
        best = np.sort(a)[:3]
        best = np.concatenate([best, np.full(3 - len(best), big, F32)]).astype(F32)
        with np.errstate(over="ignore"):
            out[i] = F32(F32(F32(best[0] + best[1]) + best[2]) / F32(3.0))
    return out


def bbox(points):
    """mean (float32, exact), radius (float64 from the float32 max - mean), min, max."""
    p = np.asarray(points, F32)
    lo, hi = p.min(0), p.max(0)
    mean = (F32(0.5) * (lo + hi).astype(F32)).astype(F32)
    d = (hi - mean).astype(F32).astype(np.float64)
    return mean, float(np.sqrt((d * d).sum())), lo, hi


def skybox_dirs(u_theta, u_phi):
    """Unit directions (S, 3), sin(phi), cos(phi): float64 from the float32 draws."""
    ut = np.asarray(u_theta, F32).astype(np.float64)
    up = np.asarray(u_phi, F32).astype(np.float64)
    theta = 2.0 * np.pi * ut
    cp = 1.0 - 1.4 * up
    sp = np.sqrt(np.maximum(1.0 - cp * cp, 0.0))
    return np.stack([np.cos(theta) * sp, np.sin(theta) * sp, cp], 1), sp, cp


def first_non_finite(points):
    """Index of the first point with a NaN or Inf coordinate, or None."""
    bad = ~np.isfinite(np.asarray(points, F32)).all(1)
    return int(np.argmax(bad)) if bad.any() else None


def init_cloud(points, colors, u_theta=None, u_phi=None, M=16, dist2=None, radius=None):
    """create_from_pcd without a scaffold_file, rows [skybox | cloud].  u_theta / u_phi None: plain
    mode (skybox_points = 0).  dist2: distCUDA2 of the (S + N) float32 positions the caller got
    (default: knn_mean_dist2 of this function's own float32-rounded positions).  radius: the float32
    radius the skybox positions are built on (default: this function's float64 one).
    Returns a dict: float32 arrays for what is exact, float64 ones (suffix 64) for the rest."""
    p = np.asarray(points, F32)
    c = np.asarray(colors, F32)
    N = p.shape[0]
    S = 0 if u_theta is None else len(u_theta)
    mean, radius64, lo, hi = bbox(p)
    out = dict(S=S, N=N, mean=mean, radius64=radius64)
    r = radius64 if radius is None else float(radius)
    xyz64 = p.astype(np.float64)
    rgb = c
    if S:
        dirs, sp, cp = skybox_dirs(u_theta, u_phi)
        sky = mean.astype(np.float64) + 10.0 * r * dirs
        xyz64 = np.concatenate([sky, xyz64])
        rgb = np.concatenate([np.tile(SKY_RGB, (S, 1)), c])
        out.update(sin_phi=sp, cos_phi=cp, r10=10.0 * r)
    out["xyz64"] = xyz64
    P = S + N
    feat = np.zeros((P, M, 3), F32)
    feat[:, 0, :] = ((rgb - F32(0.5)).astype(F32) / C0).astype(F32)
    out["features"] = feat
    if dist2 is None:
        dist2 = knn_mean_dist2(xyz64.astype(F32))
    d = np.maximum(np.asarray(dist2, F32), F32(0.0000001))
    if S:
        with np.errstate(over="ignore"):
            d[:S] = (d[:S] * F32(10.0)).astype(F32)
        d[S:] = np.minimum(d[S:], F32(10.0))
    out["d"] = d
    with np.errstate(over="ignore"):
        out["scaling64"] = np.repeat(np.log(np.sqrt(d.astype(np.float64)))[:, None], 3, 1)
    rot = np.zeros((P, 4), F32)
    rot[:, 0] = 1
    out["rotation"] = rot
    op = np.full((P, 1), logit(0.02 if S else 0.01), np.float64)
    exact = np.zeros((P, 1), bool)  # rows whose opacity is a float32 constant, to the bit
    if S:
        op[:S] = float(F32(0.7))
        exact[:S] = True
    out["opacity64"], out["opacity_exact"] = op, exact
    return out


def scaffold_select(xyz, skybox_points, center, extent, dtype=F32):
    """selec of :248-252, evaluated in `dtype` (float32: the definition; float64: for undecided()).
    hi = float32(1.5 * e0) and lo = 0.5 * e0 are the float32 constants in both."""
    x = np.asarray(xyz, F32)
    e0 = F32(np.asarray(extent, F32)[0])
    lo, hi = F32(F32(0.5) * e0), F32(F32(1.5) * e0)
    c = np.asarray(center, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        ax = np.abs((x[:, 0].astype(dtype) - dtype(c[0])).astype(dtype))
        ay = np.abs((x[:, 1].astype(dtype) - dtype(c[1])).astype(dtype))
        m = np.where(np.isnan(ax) | np.isnan(ay), dtype(np.nan), np.maximum(ax, ay))  # torch.max
        sel = (m > dtype(lo)) & (m < dtype(hi))
    sel[:int(skybox_points)] = True
    return sel


def undecided(xyz, skybox_points, center, extent):
    """Rows an fp32 evaluation could decide either way: those whose selection differs between the
    float32 definition and the same predicate with the subtractions carried out exactly (float64
    holds x - c of two float32 exactly enough: the comparison sees the unrounded distance)."""
    return scaffold_select(xyz, skybox_points, center, extent, F32) != \
        scaffold_select(xyz, skybox_points, center, extent, np.float64)


def scaffold_merge(scaffold, skybox_points, center, extent, chunk, M=16):
    """:224-264.  scaffold = (xyz (Ps,3), shs (Ps,4,3), opacity (Ps,1), scaling (Ps,3), rotation
    (Ps,4)); chunk = the same five with features (Pc, M, 3).  Returns (the five merged float32
    arrays, K, the selected indices)."""
    s = [np.asarray(a, F32) for a in scaffold]
    c = [np.asarray(a, F32) for a in chunk]
    sel = scaffold_select(s[0], skybox_points, center, extent)
    idx = np.nonzero(sel)[0]
    K = len(idx)
    shs = np.zeros((K, M, 3), F32)  # the filler of :259-260: coefficients 4.. are zero
    shs[:, :4, :] = s[1].reshape(-1, 4, 3)[idx]
    out = [np.concatenate([s[0][idx], c[0]]), np.concatenate([shs, c[1].reshape(-1, M, 3)]),
           np.concatenate([s[2].reshape(-1, 1)[idx], c[2].reshape(-1, 1)]), np.concatenate([s[3][idx], c[3]]),
           np.concatenate([s[4][idx], c[4]])]
    return out, K, idx
