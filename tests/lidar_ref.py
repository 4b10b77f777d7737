"""The rule of include/gsr_lidar.h restated in numpy: the crop, the brute-force point-to-triangle
distance and the voxel mean in float64 (the reference the GPU tests hold the kernels to), and the
kernel's distance arithmetic in float32, operation by operation in the kernel's order (what the CPU
tests measure the fp32 / fp64 gap with)."""
from __future__ import annotations

import numpy as np

F32_EPS = 2.0 ** -24


# ---- the crop ---------------------------------------------------------------------------------

def crop_bounds(center, extent):
    """x_lo, x_hi, y_lo, y_hi: c -+ e/2 with c, e and both operations in fp32."""
    c = np.asarray(center, np.float32)
    e = np.asarray(extent, np.float32)
    h = e[:2] / np.float32(2)
    return np.array([c[0] - h[0], c[0] + h[0], c[1] - h[1], c[1] + h[1]], np.float32)


def crop_mask(points, bounds):
    """Strict on both sides, x and y only; a NaN fails every comparison."""
    p = np.asarray(points, np.float32)
    with np.errstate(invalid="ignore"):
        return (bounds[0] < p[:, 0]) & (p[:, 0] < bounds[1]) & (bounds[2] < p[:, 1]) & (p[:, 1] < bounds[3])


# ---- the distance -----------------------------------------------------------------------------

def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _fma(a, b, c, dt):
    """fma in fp32 through float64 (the product of two fp32 is exact there); plain in float64."""
    if dt is np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def _diff_of_products(a, b, c, d, dt):
    w = c * d
    return _fma(a, b, -w, dt) + _fma(-c, d, w, dt)


def _seg(ux, uy, uz, ex, ey, ez, dt):
    ee = _dot(ex, ey, ez, ex, ey, ez)
    ue = _dot(ux, uy, uz, ex, ey, ez)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ee > 0, np.minimum(np.maximum(-ue / ee, dt(0)), dt(1)), dt(0)).astype(dt)
    qx, qy, qz = ux + t * ex, uy + t * ey, uz + t * ez
    return _dot(qx, qy, qz, qx, qy, qz)


def pair_d2(p, v0, v1, v2, dt):
    """d2 of gsr_lidar.h for broadcastable points p (..., 3) and triangles v0, v1, v2 (..., 3), every
    operation in dtype dt in the kernel's order; with it the per-axis minima and maxima (..., 3) of the
    three differences, which sep compares with the reach."""
    p, v0, v1, v2 = (np.asarray(a, np.float32).astype(dt) for a in (p, v0, v1, v2))
    a, b, c = v0 - p, v1 - p, v2 - p
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    bx, by, bz = b[..., 0], b[..., 1], b[..., 2]
    cx, cy, cz = c[..., 0], c[..., 1], c[..., 2]
    abx, aby, abz = bx - ax, by - ay, bz - az
    bcx, bcy, bcz = cx - bx, cy - by, cz - bz
    acx, acy, acz = cx - ax, cy - ay, cz - az
    d2 = np.minimum(_seg(ax, ay, az, abx, aby, abz, dt),
                    np.minimum(_seg(bx, by, bz, bcx, bcy, bcz, dt), _seg(ax, ay, az, acx, acy, acz, dt)))
    nx = _diff_of_products(aby, acz, abz, acy, dt)
    ny = _diff_of_products(abz, acx, abx, acz, dt)
    nz = _diff_of_products(abx, acy, aby, acx, dt)
    nn = _dot(nx, ny, nz, nx, ny, nz)
    u = _dot(nx, ny, nz, by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx)
    v = _dot(nx, ny, nz, cy * az - cz * ay, cz * ax - cx * az, cx * ay - cy * ax)
    w = _dot(nx, ny, nz, ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx)
    na = _dot(nx, ny, nz, ax, ay, az)
    with np.errstate(divide="ignore", invalid="ignore"):
        face = np.where((nn > 0) & (u >= 0) & (v >= 0) & (w >= 0), (na * na) / nn, dt(np.inf))
    d2 = np.minimum(d2, face.astype(dt))
    return d2, np.minimum(a, np.minimum(b, c)), np.maximum(a, np.maximum(b, c))


def min_d2(points, vertices, faces, dt=np.float64, reach=None, chunk=96):
    """(P,) the smallest d2 over all triangles, all pairs, in dtype dt.  Non-finite points give +Inf.
    reach (fp32, float32 runs only): triangles with sep (gsr_lidar.h) are left out, as the kernel does."""
    points = np.asarray(points, np.float32)
    v = np.asarray(vertices, np.float32)
    f = np.asarray(faces)
    v0, v1, v2 = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    out = np.full(len(points), np.inf, dt)
    ok = np.isfinite(points).all(1)
    idx = np.nonzero(ok)[0]
    for s in range(0, len(idx), chunk):
        rows = idx[s:s + chunk]
        d2, mn, mx = pair_d2(points[rows][:, None, :], v0, v1, v2, dt)
        if reach is not None:
            sep = (mn >= dt(reach)).any(-1) | (mx <= -dt(reach)).any(-1)
            d2 = np.where(sep, dt(np.inf), d2)
        out[rows] = d2.min(1)
    return out


def thresholds(max_distance):
    """(T, reach) as the library forms them: T the largest fp32 <= max_distance^2, reach an fp32 >=
    max_distance (1 + 2^-20)."""
    t2 = float(max_distance) ** 2
    T = np.float32(t2)
    if float(T) > t2:
        T = np.nextafter(T, np.float32(0))
    r = float(max_distance) * (1.0 + 2.0 ** -20)
    reach = np.float32(r)
    if float(reach) < r:
        reach = np.nextafter(reach, np.float32(np.inf))
    return T, reach


def near_mask(points, d2_64, max_distance, bounds=None):
    """The rule's mask from the float64 all-pairs d2: finite, inside the crop, distance <= max_distance."""
    points = np.asarray(points, np.float32)
    m = np.isfinite(points).all(1) & (np.sqrt(d2_64) <= float(max_distance))
    if bounds is not None:
        m &= crop_mask(points, bounds)
    return m


def near_mask_f32(points, vertices, faces, max_distance, bounds=None):
    """The kernel's own decision, all pairs: !sep && d2 <= T in fp32."""
    T, reach = thresholds(max_distance)
    d2 = min_d2(points, vertices, faces, np.float32, reach=reach)
    m = np.isfinite(np.asarray(points, np.float32)).all(1) & (d2 <= T)
    if bounds is not None:
        m &= crop_mask(points, bounds)
    return m


# ---- the voxel mean ---------------------------------------------------------------------------

def voxel_mean(points, colors, voxel_size):
    """Open3D's voxel_down_sample in float64: (means (M, 3) float32, colour means or None, counts int32,
    voxel coordinates (M, 3) int64 as ix, iy, iz), voxels in ascending (iz, iy, ix) order."""
    p = np.asarray(points, np.float32).astype(np.float64)
    s = float(voxel_size)
    if len(p) == 0:
        z = np.zeros((0, 3), np.float32)
        return z, (None if colors is None else z.copy()), np.zeros(0, np.int32), np.zeros((0, 3), np.int64)
    o = p.min(0) - s / 2.0
    top = np.floor((p.max(0) - o) / s)
    if not (top <= 2 ** 31 - 2).all():
        raise ValueError("voxel_size too small: an axis needs more than 2^31 - 1 voxels")
    ijk = np.floor((p - o) / s).astype(np.int64)
    order = np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))  # last key is the primary one; stable
    sijk = ijk[order]
    head = np.ones(len(p), bool)
    head[1:] = (sijk[1:] != sijk[:-1]).any(1)
    starts = np.nonzero(head)[0]
    counts = np.diff(np.append(starts, len(p)))
    means = np.add.reduceat(p[order], starts, axis=0) / counts[:, None]
    cmeans = None
    if colors is not None:
        c = np.asarray(colors, np.float32).astype(np.float64)
        cmeans = (np.add.reduceat(c[order], starts, axis=0) / counts[:, None]).astype(np.float32)
    return means.astype(np.float32), cmeans, counts.astype(np.int32), sijk[starts]


def ulp_diff(a, b):
    """Elementwise distance in fp32 units in the last place (finite values)."""
    def order(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(order(a) - order(b))
