"""The ray cast and encode rules of include/gsr_mesh_depth.h restated on the host, all pairs.

cast64: the rule in numpy float64 on the unrounded camera (R, C in fp64), per pixel
    distance  the smallest accepted distance over the triangles that hit (0: none),
    scale     the error scale of that hit: 2^-24 (distance + the hit triangle's largest |coordinate| in
              camera space) / |cos incidence|,
    boundary  some triangle not behind the camera has an edge function within the band of zero while
              its other two do not reject (the fp32 kernel may decide that triangle either way), or
              a decided hit's distance is within its bar of tnear or tfar,
    cands     for boundary pixels, the (distance, scale) pairs the kernel may return: the decided
              minimum (0 when no triangle is hit decidedly) and every undecided triangle's.
  The band of an edge function E(p, q) is BAND 2^-24 |d| |p| |q|: the camera-space vertices carry about
  four roundings each (C_lo, two subtractions, R's own rounding, three products and two sums), a cross
  product doubles that and adds its own, E adds three more: 16 2^-24 |d| |p| |q| bounds it; BAND = 32.
cast32: the kernel's arithmetic in numpy float32, operation by operation in its order, all pairs.
encode64: the encode in float64.
"""
from __future__ import annotations

import numpy as np

EPS = 2.0 ** -24
BAND = 32.0
RANGE_BAR = 64.0  # a decided hit within RANGE_BAR error scales of tnear / tfar is undecided


def camera64(cam):
    """R (3, 3), C (3,), fx, fy, cx, cy in float64 from the 11 doubles qvec, tvec, fx, fy, cx, cy, with
    the kernel's operation order."""
    cam = np.asarray(cam, np.float64)
    w, x, y, z = cam[:4]
    nq = np.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / nq, x / nq, y / nq, z / nq
    R = np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                  [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                  [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]], np.float64)
    t = cam[4:7]
    C = np.array([-(R[0, i] * t[0] + R[1, i] * t[1] + R[2, i] * t[2]) for i in range(3)], np.float64)
    return R, C, cam[7], cam[8], cam[9], cam[10]


def _valid_faces(vertices, faces):
    V = len(vertices)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < V)).all(1)
    f = faces[ok]
    ok2 = np.isfinite(np.asarray(vertices, np.float64)[f]).all((1, 2)) if len(f) else np.zeros(0, bool)
    return f[ok2]


def _cross(p, q):
    return np.stack([p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]], -1)


def _cross_kahan32(p, q):
    """The kernel's normal: each component x y - z w as fma(x, y, -rn(z w)) + fma(-z, w, rn(z w)).  The
    fused operations are evaluated in float64, where the product of two float32 numbers is exact (the
    sum is then rounded twice, to 53 and to 24 bits: the same result but on a 2^-29 of the inputs)."""
    f32, f64 = np.float32, np.float64

    def dop(a, b, c, d):
        w = (c * d).astype(f32)
        e = (-(c.astype(f64) * d.astype(f64)) + w.astype(f64)).astype(f32)
        f = (a.astype(f64) * b.astype(f64) - w.astype(f64)).astype(f32)
        return (f + e).astype(f32)
    return np.stack([dop(p[..., 1], q[..., 2], p[..., 2], q[..., 1]), dop(p[..., 2], q[..., 0], p[..., 0], q[..., 2]),
                     dop(p[..., 0], q[..., 1], p[..., 1], q[..., 0])], -1)


def rays(cam, W, H, dtype=np.float64):
    """(H W, 2): d_x, d_y of every pixel, row-major."""
    _, _, fx, fy, cx, cy = camera64(cam)
    T = dtype
    ix, iy = np.meshgrid(np.arange(W), np.arange(H))
    dx = ((ix.reshape(-1).astype(T) + T(0.5)) - T(cx)) / T(fx)
    dy = ((iy.reshape(-1).astype(T) + T(0.5)) - T(cy)) / T(fy)
    return dx.astype(T), dy.astype(T)


def cast64(vertices, faces, cam, W, H, tnear=0.0, tfar=1000.0, mode=0, chunk=256):
    R, C, *_ = camera64(cam)
    tn, tf = float(np.float32(tnear)), float(np.float32(tfar))
    f = _valid_faces(vertices, faces)
    v = np.asarray(vertices, np.float64)
    P = W * H
    dx, dy = rays(cam, W, H)
    dlen = np.sqrt(dx * dx + dy * dy + 1.0)
    best = np.full(P, np.inf)  # over the decided hits
    best_scale = np.zeros(P)
    rule = np.full(P, np.inf)  # over every hit of the float64 rule itself
    rule_scale = np.zeros(P)
    boundary = np.zeros(P, bool)
    cpix, cdist, cscale = [], [], []
    if len(f):
        # a triangle with two equal vertices misses whatever the rounding (gsr_mesh_depth.h): that
        # edge's function is exactly 0 and the other two are exact negatives
        t0 = v[f]
        f = f[~((t0[:, 0] == t0[:, 1]).all(1) | (t0[:, 1] == t0[:, 2]).all(1) | (t0[:, 0] == t0[:, 2]).all(1))]
    if len(f):
        tri = (v[f] - C) @ R.T  # (F, 3 vertices, 3)
        front = (tri[:, :, 2] > 0).any(1)
        tri = tri[front]
    else:
        tri = np.zeros((0, 3, 3))
    for s0 in range(0, len(tri), chunk):
        t3 = tri[s0:s0 + chunk]
        a, b, c = t3[:, 0], t3[:, 1], t3[:, 2]
        na_, nb_, nc_ = (np.linalg.norm(x, axis=1) for x in (a, b, c))
        E, band = [], []
        for (p, q, lp, lq) in ((b, c, nb_, nc_), (c, a, nc_, na_), (a, b, na_, nb_)):
            X = _cross(p, q)
            E.append(dx[:, None] * X[None, :, 0] + dy[:, None] * X[None, :, 1] + X[None, :, 2])
            band.append(BAND * EPS * dlen[:, None] * (lp * lq)[None, :])
        n = _cross(b - a, c - a)
        na = (n * a).sum(1)
        nd = dx[:, None] * n[None, :, 0] + dy[:, None] * n[None, :, 1] + n[None, :, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            s = na[None, :] / nd
            dist = s * dlen[:, None]
            cos = np.abs(nd) / (np.linalg.norm(n, axis=1)[None, :] * dlen[:, None])
            big = np.abs(t3).max((1, 2))
            scale = EPS * (np.abs(dist) + big[None, :]) / cos
        value = s if mode else dist
        pos = (E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)
        neg = (E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0)
        some = ~((E[0] == 0) & (E[1] == 0) & (E[2] == 0))
        in_range = (nd != 0) & (s > 0) & (dist > tn) & (dist <= tf)
        hit = (pos | neg) & some & in_range
        dec_pos = (E[0] > band[0]) & (E[1] > band[1]) & (E[2] > band[2])
        dec_neg = (E[0] < -band[0]) & (E[1] < -band[1]) & (E[2] < -band[2])
        near_pos = (E[0] >= -band[0]) & (E[1] >= -band[1]) & (E[2] >= -band[2])
        near_neg = (E[0] <= band[0]) & (E[1] <= band[1]) & (E[2] <= band[2])
        with np.errstate(invalid="ignore"):
            edge_on = ~(scale < np.inf)
            range_unsure = (np.abs(dist - tn) <= RANGE_BAR * scale) | (np.abs(dist - tf) <= RANGE_BAR * scale)
            # the plane's hit may be in range for the kernel: s > 0 up to the bar
            may_range = (dist > tn - RANGE_BAR * scale) & (dist <= tf + RANGE_BAR * scale) | edge_on
        undecided = ((near_pos | near_neg) & ~(dec_pos | dec_neg) & may_range) | \
                    ((dec_pos | dec_neg) & range_unsure & ~((dist == tn) | (dist == tf)) & may_range)
        decided = hit & ~undecided
        # the decided minimum
        val = np.where(decided, value, np.inf)
        j = val.argmin(1)
        rows = np.arange(P)
        better = val[rows, j] < best
        best_scale = np.where(better, scale[rows, j], best_scale)
        best = np.where(better, val[rows, j], best)
        val = np.where(hit, value, np.inf)
        j = val.argmin(1)
        better = val[rows, j] < rule
        rule_scale = np.where(better, scale[rows, j], rule_scale)
        rule = np.where(better, val[rows, j], rule)
        # the undecided triangles
        pi, ti = np.nonzero(undecided)
        if len(pi):
            boundary[pi] = True
            cpix.append(pi)
            cdist.append(np.where(np.isfinite(value[pi, ti]), value[pi, ti], 0.0))
            cscale.append(np.where(np.isfinite(scale[pi, ti]), scale[pi, ti], np.inf))
    # the float64 rule's own result on every pixel (undecided triangles decided by the float64 signs);
    # on decided pixels it is the decided minimum
    distance = np.where(np.isfinite(rule), rule, 0.0)
    decided_min = np.where(np.isfinite(best), best, 0.0)
    cands = {}
    if cpix:
        cpix, cdist, cscale = np.concatenate(cpix), np.concatenate(cdist), np.concatenate(cscale)
        order = np.argsort(cpix, kind="stable")
        cpix, cdist, cscale = cpix[order], cdist[order], cscale[order]
        cuts = np.nonzero(np.diff(cpix))[0] + 1
        for p, dd, ss in zip(np.split(cpix, cuts), np.split(cdist, cuts), np.split(cscale, cuts)):
            cands[int(p[0])] = (np.concatenate([[decided_min[p[0]]], dd]), np.concatenate([[best_scale[p[0]]], ss]))
    return {"distance": distance.reshape(H, W), "scale": rule_scale.reshape(H, W), "boundary": boundary.reshape(H, W),
            "cands": cands}


def camera32(cam):
    """The fp32 camera record: R, C_hi, C_lo, fx, fy, cx, cy."""
    R, C, fx, fy, cx, cy = camera64(cam)
    f = np.float32
    chi = C.astype(f)
    clo = (C - chi.astype(np.float64)).astype(f)
    return R.astype(f), chi, clo, f(fx), f(fy), f(cx), f(cy)


def cast32(vertices, faces, cam, W, H, tnear=0.0, tfar=1000.0, mode=0, chunk=256):
    """(H, W) float32: the kernel's arithmetic, all pairs."""
    f32 = np.float32
    R, chi, clo, fx, fy, cx, cy = camera32(cam)
    tn, tf = f32(tnear), f32(tfar)
    fc = _valid_faces(vertices, faces)
    v = np.asarray(vertices, f32)
    P = W * H
    ix, iy = np.meshgrid(np.arange(W), np.arange(H))
    dx = ((ix.reshape(-1).astype(f32) + f32(0.5)) - cx) / fx
    dy = ((iy.reshape(-1).astype(f32) + f32(0.5)) - cy) / fy
    dlen = np.sqrt((dx * dx + dy * dy) + f32(1))
    best = np.full(P, np.inf, f32)
    with np.errstate(all="ignore"):
        e = (v - chi) - clo  # (V, 3)
        cs = np.stack([(R[r, 0] * e[:, 0] + R[r, 1] * e[:, 1]) + R[r, 2] * e[:, 2] for r in range(3)], 1)
        tri = cs[fc] if len(fc) else np.zeros((0, 3, 3), f32)
        tri = tri[np.isfinite(tri).all((1, 2))]

        def edge(p, q):
            swap = (q[:, 0] < p[:, 0]) | ((q[:, 0] == p[:, 0]) & ((q[:, 1] < p[:, 1]) | ((q[:, 1] == p[:, 1]) & (q[:, 2] < p[:, 2]))))
            lo = np.where(swap[:, None], q, p)
            hi = np.where(swap[:, None], p, q)
            X = _cross(lo, hi)
            return np.where(swap[:, None], -X, X)

        for s0 in range(0, len(tri), chunk):
            t3 = tri[s0:s0 + chunk]
            a, b, c = t3[:, 0], t3[:, 1], t3[:, 2]
            E = []
            for X in (edge(b, c), edge(c, a), edge(a, b)):
                E.append((dx[:, None] * X[None, :, 0] + dy[:, None] * X[None, :, 1]) + X[None, :, 2])
            n = _cross_kahan32(b - a, c - a)
            na = (n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2]
            nd = (n[None, :, 0] * dx[:, None] + n[None, :, 1] * dy[:, None]) + n[None, :, 2]
            s = na[None, :] / nd
            t = s * dlen[:, None]
            assert s.dtype == f32 and t.dtype == f32 and E[0].dtype == f32
            pos = (E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)
            neg = (E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0)
            some = ~((E[0] == 0) & (E[1] == 0) & (E[2] == 0))
            hit = (pos | neg) & some & (nd != 0) & (s > 0) & (tn < t) & (t <= tf)
            best = np.minimum(best, np.where(hit, s if mode else t, f32(np.inf)).min(1))
    return np.where(np.isfinite(best), best, f32(0)).reshape(H, W).astype(f32)


def margin_units(d32, r64):
    """The largest |d32 - distance| / scale over the decided pixels of a cast64 result, and whether
    hit / miss agrees on all of them."""
    dec = ~r64["boundary"]
    hit64 = r64["distance"] > 0
    same = bool(((d32 > 0) == hit64)[dec].all())
    m = dec & hit64 & (d32 > 0)
    if not m.any():
        return 0.0, same
    return float((np.abs(d32.astype(np.float64) - r64["distance"])[m] / r64["scale"][m]).max()), same


def judge(got, r64, bar_units, closed=None):
    """Problems (strings) of a (H, W) float32 result against a cast64 result under a bar of bar_units
    error scales: decided pixels by distance, boundary pixels by their candidates.  closed: (H, W) bool,
    the pixels whose ray cannot miss: 0 is no candidate there."""
    H, W = got.shape
    if closed is None:
        closed = np.zeros((H, W), bool)
    bad = []
    g = got.astype(np.float64)
    dec = ~r64["boundary"]
    hit = r64["distance"] > 0
    wrong = dec & ((g > 0) != hit)
    if wrong.any():
        bad.append(f"{int(wrong.sum())} decided pixels differ in hit / miss, first {tuple(np.argwhere(wrong)[0])}")
    m = dec & hit & (g > 0)
    err = np.zeros_like(g)
    err[m] = np.abs(g - r64["distance"])[m] / r64["scale"][m]
    if (err > bar_units).any():
        bad.append(f"decided distance off by {err.max():.2f} error scales (bar {bar_units:.2f}) at "
                   f"{tuple(np.argwhere(err == err.max())[0])}")
    for p, (cd, cs) in r64["cands"].items():
        val = g[p // W, p % W]
        ok = False
        for d, s in zip(cd, cs):
            if d == 0:
                ok = ok or (val == 0 and not closed[p // W, p % W])
            else:
                ok = ok or (val > 0 and abs(val - d) <= bar_units * s)
        if cd[0] > 0 and not (0 < val <= cd[0] + bar_units * cs[0]):  # never behind a decided hit
            ok = False
        if not ok:
            bad.append(f"boundary pixel {(p // W, p % W)}: {val} matches none of {cd.tolist()[:6]}")
    holes = closed & (got == 0)
    if holes.any():
        bad.append(f"{int(holes.sum())} holes in a closed surface, first {tuple(np.argwhere(holes)[0])}")
    return bad


# ---- the encode ----------------------------------------------------------------------------------------

def depth_of_mm(mm):
    """(depth float64, background bool) of float64 millimetres under the 3-channel code and its decode."""
    mm = np.asarray(mm, np.float64)
    with np.errstate(invalid="ignore"):
        bg = ~(mm >= 1.0) | (mm > 1048576.0)
    m = np.where(bg, 1.0, mm)
    sh = np.where(m <= 65536.0, 2, np.where(m <= 262144.0, 4, 6)).astype(np.int64)
    units = np.floor(m / (1 << sh).astype(np.float64)).astype(np.int64)
    depth = ((units & 0x3FFF) << sh).astype(np.float64) / 1000.0
    return np.where(bg, 0.0, depth), bg


def depth_of(dist, quantize):
    """(depth float64, background bool) of float32 distances."""
    d = np.asarray(dist, np.float32)
    if not quantize:
        return d.astype(np.float64), d == 0
    return depth_of_mm(1000.0 * d.astype(np.float64))


def normalise64(depth, bg, min_depth=0.1, max_depth=None):
    """(u16 (H, W) uint16, scale, offset) of one image's depths and background mask."""
    u16 = np.zeros(depth.shape, np.uint16)
    with np.errstate(invalid="ignore"):
        valid = ~bg & (depth > min_depth)
        if max_depth is not None:
            valid &= depth < max_depth
    if not valid.any():
        return u16, 0.0, 0.0
    inv = np.zeros_like(depth)
    inv[valid] = 1.0 / depth[valid]
    lo, hi = inv[valid].min(), inv[valid].max()
    if not hi > lo:
        return u16, 0.0, float(lo)
    scale = hi - lo
    x = np.zeros_like(depth)
    x[valid] = (inv[valid] - lo) / scale
    return (np.clip(x, 0.0, 1.0) * 65535).astype(np.uint16), float(scale), float(lo)


def encode64(dist, quantize=True, min_depth=0.1, max_depth=None):
    """(u16 (K, H, W) uint16, scale (K,), offset (K,)) of (K, H, W) float32 distances."""
    dist = np.asarray(dist, np.float32)
    K = dist.shape[0]
    u16 = np.zeros(dist.shape, np.uint16)
    scale, offset = np.zeros(K), np.zeros(K)
    for k in range(K):
        depth, bg = depth_of(dist[k], quantize)
        u16[k], scale[k], offset[k] = normalise64(depth, bg, min_depth, max_depth)
    return u16, scale, offset


def code_steps(quantize_input):
    """The distance (float64, metres) from a float32 quantiser input to the nearest code step: a
    multiple of the band's step, or a band limit."""
    mm = 1000.0 * np.asarray(quantize_input, np.float64)
    step = np.where(mm <= 65536.0, 4.0, np.where(mm <= 262144.0, 16.0, 64.0))
    r = np.mod(mm, step)
    near = np.minimum(r, step - r)
    for lim in (1.0, 65536.0, 262144.0, 1048576.0):
        near = np.minimum(near, np.abs(mm - lim))
    return near / 1000.0
