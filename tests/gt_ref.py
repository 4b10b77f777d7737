"""numpy reference of the ground-truth cloud constraint (include/gsr_gtcloud.h): a chunked all-pairs
evaluation of the d2 rule in float32.

    inside = x >= x_min && x <= x_max && y >= y_min && y <= y_max      (fp32, inclusive, no z test)
    d2     = (dx*dx + dy*dy) + dz*dz,  d = g - p, every operation rounded to float32
    D      = inside && all over the cloud of ((double)d2 > thr*thr)

numpy's float32 array arithmetic rounds each operation to float32 and never contracts, so this is
the rule bit for bit.  Comparisons with NaN are false: a NaN x or y is outside, a NaN z gives D = 0;
an infinite z gives d2 = +Inf for every point, so D = 1 when inside."""
from __future__ import annotations

import numpy as np


def bounds(cloud):
    """x_min, x_max, y_min, y_max as load_gt_point_cloud computes them (float32 min / max)."""
    c = np.asarray(cloud, np.float32)
    return np.min(c[:, 0]), np.max(c[:, 0]), np.min(c[:, 1]), np.max(c[:, 1])


def inside_bounds(xyz, cloud):
    x_min, x_max, y_min, y_max = bounds(cloud)
    p = np.asarray(xyz, np.float32)
    with np.errstate(invalid="ignore"):
        return (p[:, 0] >= x_min) & (p[:, 0] <= x_max) & (p[:, 1] >= y_min) & (p[:, 1] <= y_max)


def min_d2(xyz, cloud, chunk_pairs=1 << 22):
    """The float32 minimum over the cloud of d2 per row of xyz (NaN where any d2 is NaN)."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    c = np.asarray(cloud, np.float32).reshape(-1, 3)
    out = np.empty(p.shape[0], np.float32)
    rows = max(1, chunk_pairs // max(c.shape[0], 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(0, p.shape[0], rows):
            q = p[s:s + rows]
            dx = c[None, :, 0] - q[:, None, 0]
            dy = c[None, :, 1] - q[:, None, 1]
            dz = c[None, :, 2] - q[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            out[s:s + rows] = d2.min(axis=1)  # numpy's min propagates NaN
    return out


def far_mask(xyz, cloud, thr, skip=None):
    """D per row (bool); rows with skip set get False."""
    p = np.asarray(xyz, np.float32).reshape(-1, 3)
    m = inside_bounds(p, cloud)
    if skip is not None:
        m &= ~np.asarray(skip, bool)
    out = np.zeros(p.shape[0], bool)
    idx = np.nonzero(m)[0]
    if idx.size:
        d = min_d2(p[idx], cloud)
        with np.errstate(invalid="ignore"):
            # every d2 > thr^2  <=>  the minimum is (NaN: some comparison fails)
            out[idx] = d.astype(np.float64) > float(thr) * float(thr)
    return out


def compare_points_to_gt(xyz, cloud, thr, existing=None, protected=None):
    """The reference's combined mask: existing | D, D skipped on existing and protected rows."""
    P = np.asarray(xyz).reshape(-1, 3).shape[0]
    skip = np.zeros(P, bool)
    if existing is not None:
        skip |= np.asarray(existing, bool)
    if protected is not None:
        skip |= np.asarray(protected, bool)
    far = far_mask(xyz, cloud, thr, skip)
    return far if existing is None else np.asarray(existing, bool) | far
