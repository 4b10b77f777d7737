"""numpy restatement of the LOD hierarchy builder's rule (DESIGN.md "Hierarchy builder", rules A-E),
the checker of csrc/hier_build.hip -- test infrastructure, as tests/gt_ref.py is for the ground-truth
cloud.  The rule is this project's definition (Kerbl et al. 2024 sec. 5 over an LBVH; parity unpinned
against the un-vendored gaussianhierarchy tool).  Integer parts (keys, order, topology, layout) are
exact: python integers and correctly rounded float64 operations.  Attribute maths is float64 with
np.linalg.eigh for the decomposition; `merge_step(..., dtype=np.float32)` evaluates the same step in
float32, the basis of the GPU test's tolerances.
"""
from __future__ import annotations

import numpy as np

SURFACE_P = 1.6075
MIN_EIGEN = 1e-14


# ---- A. order ----------------------------------------------------------------------------------

def _spread21(x):
    x = x & np.uint64(0x1FFFFF)
    x = (x | (x << np.uint64(32))) & np.uint64(0x1F00000000FFFF)
    x = (x | (x << np.uint64(16))) & np.uint64(0x1F0000FF0000FF)
    x = (x | (x << np.uint64(8))) & np.uint64(0x100F00F00F00F00F)
    x = (x | (x << np.uint64(4))) & np.uint64(0x10C30C30C30C30C3)
    x = (x | (x << np.uint64(2))) & np.uint64(0x1249249249249249)
    return x


def morton_keys(xyz):
    """63-bit keys (uint64) of fp32 positions: one cube scale, 2^21 cells per axis, x in bit 0."""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    lo, hi = x.min(0), x.max(0)  # fp32
    ext = float(np.max(hi.astype(np.float64) - lo.astype(np.float64)))
    if not ext > 0:
        return np.zeros(x.shape[0], np.uint64)
    t = np.floor((x.astype(np.float64) - lo.astype(np.float64)) * (2097152.0 / ext))
    q = np.minimum(np.float64(2 ** 21 - 1), t).astype(np.uint64)
    return _spread21(q[:, 0]) | (_spread21(q[:, 1]) << np.uint64(1)) | (_spread21(q[:, 2]) << np.uint64(2))


def sorted_order(keys):
    """Input rows ascending by (key, row)."""
    return np.lexsort((np.arange(keys.shape[0]), keys))


# ---- B. topology -------------------------------------------------------------------------------

def delta(skeys, a, b):
    """skeys: the sorted keys as python integers; a != b sorted positions."""
    ka, kb = skeys[a], skeys[b]
    if ka != kb:
        return 64 - (ka ^ kb).bit_length()
    return 64 + 32 - (a ^ b).bit_length()


def split(skeys, f, l):
    """The largest g in [f, l) with g == f or delta(f, g) > delta(f, l) (delta(f, .) does not
    increase along the sorted leaves, so a bisection finds it)."""
    dn = delta(skeys, f, l)
    lo, hi = f, l - 1  # the answer is in [lo, hi]; lo always satisfies the condition
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if delta(skeys, f, mid) > dn:
            lo = mid
        else:
            hi = mid - 1
    return lo


def split_by_scan(skeys, f, l):
    """The same by the definition, without the monotonicity argument (small inputs)."""
    dn = delta(skeys, f, l)
    return max(g for g in range(f, l) if g == f or delta(skeys, f, g) > dn)


# ---- C. layout ---------------------------------------------------------------------------------

def topology(keys, split_fn=split):
    """nodes (N, 7) int32, leaf_rows (N) int32 and the level count of P keys, N = 2 P - 1."""
    P = keys.shape[0]
    order = sorted_order(keys)
    skeys = [int(k) for k in keys[order]]
    N = 2 * P - 1
    nodes = np.zeros((N, 7), np.int32)
    leaf_rows = np.full(N, -1, np.int32)
    ranges = [(0, P - 1)]  # breadth-first: node n's leaf range, appended as its parent is visited
    nodes[0, :2] = (0, -1)
    for n in range(N):
        f, l = ranges[n]
        nodes[n, 2] = n
        if f == l:
            nodes[n, 3:] = (1, 0, -1, 0)
            leaf_rows[n] = order[f]
            continue
        g = split_fn(skeys, f, l)
        c = len(ranges)
        ranges += [(f, g), (g + 1, l)]
        nodes[n, 3:] = (0, 1, c, 2)
        nodes[c:c + 2, 0] = nodes[n, 0] + 1
        nodes[c:c + 2, 1] = n
    assert len(ranges) == N
    return nodes, leaf_rows, int(nodes[:, 0].max()) + 1


# ---- D, E. attributes --------------------------------------------------------------------------

def quat_to_rot(q):
    """(K, 3, 3) rotation of unit quaternions (r, x, y, z): the rasterizer's convention."""
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = q.dtype.type(1), q.dtype.type(2)
    R = np.empty((q.shape[0], 3, 3), q.dtype)
    R[:, 0, 0] = one - two * (y * y + z * z)
    R[:, 0, 1] = two * (x * y - r * z)
    R[:, 0, 2] = two * (x * z + r * y)
    R[:, 1, 0] = two * (x * y + r * z)
    R[:, 1, 1] = one - two * (x * x + z * z)
    R[:, 1, 2] = two * (y * z - r * x)
    R[:, 2, 0] = two * (x * z - r * y)
    R[:, 2, 1] = two * (y * z + r * x)
    R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def rot_to_quat(m):
    """Unit quaternions (r, x, y, z) of (K, 3, 3) proper rotations; the branch with the largest divisor."""
    dt = m.dtype.type
    tr = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
    cand = np.stack([dt(1) + tr, dt(1) + m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2],
                     dt(1) - m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2], dt(1) - m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]], 1)
    k = np.argmax(cand, 1)
    s = dt(2) * np.sqrt(np.maximum(cand[np.arange(m.shape[0]), k], dt(1e-30)))  # 4 |the largest component|
    a, b, c = m[:, 2, 1] - m[:, 1, 2], m[:, 0, 2] - m[:, 2, 0], m[:, 1, 0] - m[:, 0, 1]
    d, e, f = m[:, 0, 1] + m[:, 1, 0], m[:, 0, 2] + m[:, 2, 0], m[:, 1, 2] + m[:, 2, 1]
    q4 = s * dt(0.25)
    table = [np.stack([q4, a / s, b / s, c / s], 1), np.stack([a / s, q4, d / s, e / s], 1),
             np.stack([b / s, d / s, q4, f / s], 1), np.stack([c / s, e / s, f / s, q4], 1)]
    q = np.choose(k[:, None], table)
    return q / np.sqrt((q * q).sum(1, keepdims=True))


def row_cov(log_scales, rotations):
    """Sigma = R diag(s^2) R^T of stored rows, s = exp(log-scale), R from q / |q|; also s."""
    s = np.exp(log_scales)
    q = rotations / np.sqrt((rotations * rotations).sum(1, keepdims=True))
    R = quat_to_rot(q)
    return np.einsum("kij,kj,klj->kil", R, s * s, R), s


def surface(s):
    """Thomsen's ellipsoid surface without the 4 pi."""
    p = s.dtype.type(SURFACE_P)
    t = (np.power(s[:, 0] * s[:, 1], p) + np.power(s[:, 0] * s[:, 2], p) + np.power(s[:, 1] * s[:, 2], p))
    return np.power(t / s.dtype.type(3), s.dtype.type(1) / p)


def leaf_box(xyz, log_scales, rotations):
    """(minn, maxx) = mu -+ 3 sqrt(diag Sigma), in the inputs' dtype."""
    cov, _ = row_cov(log_scales, rotations)
    h = xyz.dtype.type(3) * np.sqrt(np.stack([cov[:, 0, 0], cov[:, 1, 1], cov[:, 2, 2]], 1))
    return xyz - h, xyz + h


def merge_step(a, b, dtype=np.float64):
    """Rule E for K pairs of child rows.  a, b: dicts of xyz (K,3), log_scales (K,3), rotations (K,4),
    opacities (K), shs (K, 3M); every operation in `dtype`.  Returns xyz, log_scales, rotations,
    opacities, shs of the merged rows and W, cov (the mixture covariance before the decomposition)."""
    A = {k: np.asarray(v).astype(dtype) for k, v in a.items()}
    B = {k: np.asarray(v).astype(dtype) for k, v in b.items()}
    dt = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        ca, sa = row_cov(A["log_scales"], A["rotations"])
        cb, sb = row_cov(B["log_scales"], B["rotations"])
        wa, wb = A["opacities"] * surface(sa), B["opacities"] * surface(sb)
        W = wa + wb
        ok = np.isfinite(W) & (W > 0)
        Ws = np.where(ok, W, dt(1))
        ua, ub = np.where(ok, wa / Ws, dt(0.5)), np.where(ok, wb / Ws, dt(0.5))
        mu = ua[:, None] * A["xyz"] + ub[:, None] * B["xyz"]
        shs = ua[:, None] * A["shs"] + ub[:, None] * B["shs"]
        da, db = A["xyz"] - mu, B["xyz"] - mu
        cov = (ua[:, None, None] * (ca + da[:, :, None] * da[:, None, :])
               + ub[:, None, None] * (cb + db[:, :, None] * db[:, None, :]))
        lam, V = np.linalg.eigh(cov)
        lam = np.maximum(lam, dt(MIN_EIGEN))
        V = V * np.where(np.linalg.det(V) < 0, dt(-1), dt(1))[:, None, None]  # odd dimension: -V is proper
        sm = np.sqrt(lam)
        op = np.where(ok, Ws / surface(sm), dt(0))
    return dict(xyz=mu, log_scales=np.log(sm), rotations=rot_to_quat(V), opacities=op, shs=shs, W=W, cov=cov)


def build(xyz, log_scales, rotations, opacities, shs):
    """The hierarchy of P rows: nodes, leaf_rows, levels (exact) and the N rows' attributes in
    float64: means3D, log_scales, rotations, opacities (N), shs (N, M, 3), boxes (N, 2, 4), W (N: a
    leaf's o S(s), an interior node's w_a + w_b)."""
    xyz32 = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    P = xyz32.shape[0]
    M = np.asarray(shs).shape[1]
    nodes, leaf_rows, levels = topology(morton_keys(xyz32))
    N = nodes.shape[0]
    src = dict(xyz=xyz32, log_scales=np.asarray(log_scales).reshape(P, 3), rotations=np.asarray(rotations).reshape(P, 4),
               opacities=np.asarray(opacities).reshape(P), shs=np.asarray(shs).reshape(P, 3 * M))
    out = {k: np.zeros((N,) + v.shape[1:], np.float64) for k, v in src.items()}
    leaf = leaf_rows >= 0
    for k, v in src.items():
        out[k][leaf] = v[leaf_rows[leaf]].astype(np.float64)
    mn, mx = np.zeros((N, 3)), np.zeros((N, 3))
    mn[leaf], mx[leaf] = leaf_box(out["xyz"][leaf], out["log_scales"][leaf], out["rotations"][leaf])
    W = np.zeros(N)
    W[leaf] = out["opacities"][leaf] * surface(np.exp(out["log_scales"][leaf]))
    for d in range(levels - 2, -1, -1):  # children before parents
        idx = np.nonzero((nodes[:, 0] == d) & ~leaf)[0]
        ca = nodes[idx, 5]
        m = merge_step({k: v[ca] for k, v in out.items()}, {k: v[ca + 1] for k, v in out.items()})
        for k in out:
            out[k][idx] = m[k]
        W[idx] = m["W"]
        # the union in fp32, as the rule states it (the leaves' boxes rounded once)
        mn[idx] = np.minimum(mn[ca].astype(np.float32), mn[ca + 1].astype(np.float32))
        mx[idx] = np.maximum(mx[ca].astype(np.float32), mx[ca + 1].astype(np.float32))
    boxes = np.zeros((N, 2, 4))
    boxes[:, 0, :3], boxes[:, 1, :3] = mn, mx
    boxes[:, 0, 3] = box_extent(boxes.astype(np.float32))
    return dict(nodes=nodes, leaf_rows=leaf_rows, levels=levels, means3D=out["xyz"], log_scales=out["log_scales"],
                rotations=out["rotations"], opacities=out["opacities"], shs=out["shs"].reshape(N, M, 3), boxes=boxes,
                W=W)


def box_extent(boxes32):
    """boxes[:, 0, 3] of fp32 boxes: the largest fp32 extent."""
    b = np.asarray(boxes32, np.float32)
    return (b[:, 1, :3] - b[:, 0, :3]).max(1)


# ---- error measures of one merge (per node), used with 4 x the fp32 evaluation's error ------------

def cov_of_rows(log_scales, rotations):
    return row_cov(np.asarray(log_scales, np.float64), np.asarray(rotations, np.float64))[0]


def step_errors(got, ref, a, b):
    """Largest error of merged rows `got` (any dtype) against the float64 step `ref` of the children a, b:
    mu and SH relative to the larger child norm, opacity relative, and R diag(s^2) R^T of the stored
    log-scales and quaternion against the mixture covariance in relative Frobenius norm."""
    f = lambda x: np.asarray(x, np.float64)
    n2 = lambda x: np.sqrt((f(x) ** 2).sum(axis=tuple(range(1, np.ndim(x)))))
    tiny = 1e-300
    mu = n2(f(got["xyz"]) - ref["xyz"]) / np.maximum(np.maximum(n2(a["xyz"]), n2(b["xyz"])), tiny)
    sh = n2(f(got["shs"]) - ref["shs"]) / np.maximum(np.maximum(n2(a["shs"]), n2(b["shs"])), tiny)
    ro = ref["opacities"]
    op = np.abs(f(got["opacities"]) - ro) / np.where(ro > 0, ro, 1.0)
    cov = n2(cov_of_rows(got["log_scales"], got["rotations"]) - ref["cov"]) / np.maximum(n2(ref["cov"]), tiny)
    worst = lambda e: float(e.max()) if e.size else 0.0
    return dict(mu=worst(mu), sh=worst(sh), opacity=worst(op), cov=worst(cov))


def leaf_box_error(minn, maxx, xyz, log_scales, rotations):
    """Largest coordinate error of leaf boxes against float64, relative to the box's largest coordinate."""
    f = lambda x: np.asarray(x, np.float64)
    mn, mx = leaf_box(f(xyz), f(log_scales), f(rotations))
    err = np.maximum(np.abs(f(minn) - mn).max(1), np.abs(f(maxx) - mx).max(1))
    mag = np.maximum(np.abs(mn).max(1), np.abs(mx).max(1))
    return float((err / np.maximum(mag, 1e-300)).max())


# ---- the test problems (shared by the CPU and the GPU tests) ---------------------------------------

def cloud(kind, P, M=16, seed=0):
    """P rows in synthetic.camera's frustum (fp32): positions by `kind` -- "random", "ties" (a third of
    the rows at one of four positions), "planar" (all z equal), "identical" (one position: ext = 0),
    "zero_pair" (random, the opacities of the first half zero, so some merges have W = 0) -- log-scales
    ~ N(-4, 0.5) with a third of the rows flattened along one axis (a street's surfaces), raw
    quaternions of any length, activated opacities, SH."""
    from gs_train.synthetic import camera
    rng = np.random.default_rng(seed)
    _, _, _, tx, ty = camera(640, 360)
    z = rng.uniform(2.0, 20.0, P)
    xyz = np.stack([rng.uniform(-0.95, 0.95, P) * tx * z, rng.uniform(-0.95, 0.95, P) * ty * z, z], 1)
    if kind == "ties":
        spots = xyz[:4].copy()
        rows = rng.permutation(P)[:max(P // 3, min(P, 2))]
        xyz[rows] = spots[rng.integers(0, min(4, P), rows.shape[0])]
    elif kind == "planar":
        xyz[:, 2] = 7.5
    elif kind == "identical":
        xyz[:] = xyz[0]
    elif kind not in ("random", "zero_pair"):
        raise ValueError(kind)
    ls = rng.normal(-4.0, 0.5, (P, 3))
    flat = rng.random(P) < 1 / 3
    ls[flat, rng.integers(0, 3, int(flat.sum()))] -= 3.0
    q = rng.normal(size=(P, 4))
    q *= rng.uniform(0.5, 2.0, (P, 1)) / np.linalg.norm(q, axis=1, keepdims=True)
    op = rng.uniform(0.05, 0.99, (P, 1))
    if kind == "zero_pair":
        op[:max(P // 2, min(P, 2))] = 0.0
    shs = rng.normal(0, 0.05, (P, M, 3))
    shs[:, 0] = rng.normal(0, 0.5, (P, 3))
    f = lambda x: np.ascontiguousarray(x, np.float32)
    return dict(xyz=f(xyz), log_scales=f(ls), rotations=f(q), opacities=f(op), shs=f(shs))


def children_of(h, rows32=True):
    """The (a, b) child-row dicts of every interior node of a built hierarchy `h` (build()'s dict or the
    device's arrays as numpy), and the interior node ids; rows32: the rows rounded to fp32 first."""
    nodes = np.asarray(h["nodes"])
    idx = np.nonzero(nodes[:, 6] == 2)[0]
    ca = nodes[idx, 5]
    N = nodes.shape[0]
    conv = (lambda x: np.asarray(x, np.float32)) if rows32 else np.asarray
    rows = dict(xyz=conv(h["means3D"]).reshape(N, 3), log_scales=conv(h["log_scales"]).reshape(N, 3),
                rotations=conv(h["rotations"]).reshape(N, 4), opacities=conv(h["opacities"]).reshape(N),
                shs=conv(h["shs"]).reshape(N, -1))
    return idx, {k: v[ca] for k, v in rows.items()}, {k: v[ca + 1] for k, v in rows.items()}, rows


# the GPU test's build problems: (kind, P, M); the seed is P
GPU_CASES = [("random", 1, 16), ("random", 2, 16), ("random", 3, 4), ("random", 64, 16), ("random", 65, 4),
             ("random", 1000, 4), ("random", 4097, 16), ("ties", 300, 16), ("planar", 300, 16), ("identical", 300, 16),
             ("zero_pair", 300, 4), ("random", 20000, 16)]


def fp32_basis(cases=GPU_CASES):
    """The basis of the GPU test's tolerances: the largest error a float32 numpy evaluation of rule E
    (and of the leaf box) shows against float64 on the cases' own rows -- every interior node's two
    child rows of the reference-built hierarchy, rounded to fp32 as a device holds them."""
    worst = dict(mu=0.0, sh=0.0, opacity=0.0, cov=0.0, leaf_box=0.0)
    for kind, P, M in cases:
        c = cloud(kind, P, M, seed=P)
        h = build(**c)
        _, a, b, _ = children_of(h)
        e = step_errors(merge_step(a, b, np.float32), merge_step(a, b), a, b)
        mn, mx = leaf_box(c["xyz"], c["log_scales"], c["rotations"])  # float32 inputs: a float32 evaluation
        e["leaf_box"] = leaf_box_error(mn, mx, c["xyz"], c["log_scales"], c["rotations"])
        worst = {k: max(v, e[k]) for k, v in worst.items()}
    return worst


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "street-sparse-3dgs_amd"))
    for k, v in fp32_basis().items():
        print(f"{k}: measured {v:.3e}  bound (4x) {4 * v:.3e}")
