"""TEST INFRASTRUCTURE ONLY -- float64 numpy reference of the hierarchy-cut blend (csrc/hier.hip,
include/gsr_hier.h) with per-element error scales, and of the blend-weight rule of csrc/lod.hip.

A case is a dict (tests/cut_cases.py): N, M, S, the five float32 arrays xyz (N, 3), scaling (N, 3),
rotation (N, 4), opacity (N, 1), features (N, M, 3), and ri / pi (int32, R) / w (float32, R).  `act`
selects the form: 0 = the arrays are activated values (gsr_interpolate_cut_forward), 1 / 2 = they are the
raw parameters and exp, F.normalize (eps 1e-12) and sigmoid / abs are applied to the rows the cut reads
(gsr_interpolate_cut_forward_act).  Roots (parent -1) read and write row N - 1.

Every function takes the dtype it computes in.  float64 is the reference; float32 restates the kernels'
order of operations (the dot left to right, t a + (1 - t) b, normalize's (x / d) / d) on the host, which
is what the bars of the raw form are measured from (tests/test_cut_cases_cpu.py).

Error scales, per element:
  forward   fwd_scale = |t a| + |(1 - t) b|: the blend is four roundings (1 - t, two products, a sum),
            so |err| <= 4 * 2^-24 * fwd_scale when a and b are exact (the activated form).
  backward  a gradient element is a sum of grad_cnt terms of total size grad_abs = sum |term|: a float32
            sum in any order (the atomics) of terms each rounded twice is within
            (grad_cnt + 2) * 2^-24 * grad_abs.  A term's size is taken after its chain factor:
              exp        |g e^s|
              abs        |g|
              sigmoid    |g| y ((1 - y) + |1 - 2 y|): the factor y (1 - y) is formed from the rounded y,
                         whose relative error enters 1 - y absolutely -- at y -> 1 the factor itself
                         vanishes while its error does not
              normalize  |g_k| / d + |x_k| sum_j |g_j x_j| / (d^2 n): the two terms of
                         g / d - x (g . x) / (d^2 n), which cancel
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24  # float32 unit roundoff
NORM_EPS = 1e-12
FIELDS = ("xyz", "scaling", "rotation", "opacity", "features")
OUTS = ("means3D", "scales", "rotations", "opacities", "shs")
SIGMOID, ABS = 1, 2


def rows(c):
    """(child, parent, t, live) of the R + S output rows; live = blended (not a skybox copy)."""
    N, S = int(c["N"]), int(c["S"])
    ri = np.asarray(c["ri"], np.int64)
    R = len(ri)
    pi = np.asarray(c["pi"], np.int64)[:R]
    pi = np.where(pi < 0, pi + N, pi)
    sky = np.arange(N - S, N, dtype=np.int64)
    t = np.concatenate([np.asarray(c["w"], np.float32)[:R], np.ones(S, np.float32)])
    live = np.concatenate([np.ones(R, bool), np.zeros(S, bool)])
    return np.concatenate([ri, sky]), np.concatenate([pi, sky]), t, live


def _norm(q):
    return np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])[:, None]


def activate(c, act, dt=np.float64):
    """The five arrays the blend reads, in dt: [means, scales, rotations, opacities, shs]."""
    x, s, q, o, sh = (np.asarray(c[k]).astype(dt) for k in FIELDS)
    if act == 0:
        return [x, s, q, o, sh]
    with np.errstate(over="ignore"):
        oa = np.abs(o) if act == ABS else dt(1) / (dt(1) + np.exp(-o))
    return [x, np.exp(s), q / np.maximum(_norm(q), dt(NORM_EPS)), oa, sh]


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2] + a[:, 3] * b[:, 3]


def rotation_dots(c, act, dt=np.float64):
    """Per output row: the dot of the child's and the parent's (activated) rotation, left to right,
    and sum |q_c,k q_p,k|."""
    ch, pa, _, _ = rows(c)
    q = activate(c, act, dt)[2]
    return _dot(q[ch], q[pa]), _dot(np.abs(q[ch]), np.abs(q[pa]))


def _bc(v, a):
    return v.reshape((-1,) + (1,) * (a.ndim - 1))


def forward(c, act=0, dt=np.float64):
    """-> (outs, scales): two dicts over OUTS of (R + S)-row arrays in dt."""
    ch, pa, t, live = rows(c)
    t = t.astype(dt)
    u = dt(1) - t
    arrs = activate(c, act, dt)
    sgn = np.where(_dot(arrs[2][ch], arrs[2][pa]) < 0, dt(-1), dt(1))
    outs, scales = {}, {}
    for k, name in enumerate(OUTS):
        a, b = arrs[k][ch], arrs[k][pa]
        if name == "rotations":
            b = b * sgn[:, None]
        lv = _bc(live, a)
        outs[name] = np.where(lv, _bc(t, a) * a + _bc(u, a) * b, a)
        scales[name] = np.where(lv, np.abs(_bc(t, a) * a) + np.abs(_bc(u, a) * b), np.abs(a))
    return outs, scales


def _normalize_grad(x, g, dt):
    """F.normalize's backward at the raw rows x for the upstream rows g, as torch clamps it (no gradient
    through the norm below eps or at 0), and the size of its two terms."""
    n = _norm(x)
    d = np.maximum(n, dt(NORM_EPS))
    xd = (x / d) / d
    gd = -(g[:, 0] * xd[:, 0] + g[:, 1] * xd[:, 1] + g[:, 2] * xd[:, 2] + g[:, 3] * xd[:, 3])[:, None]
    through = (n >= dt(NORM_EPS)) & (n != 0)
    safe = np.where(through, n, dt(1))
    gn = np.where(through, gd / safe, dt(0))
    size = np.abs(g) / d + np.where(through, np.abs(x) * (np.abs(g) * np.abs(xd)).sum(1, keepdims=True) / safe, dt(0))
    return g / d + x * gn, size


def backward(c, ups, act=0, dt=np.float64):
    """ups: five (R + S)-row upstream gradients over OUTS, or None for a zero one.
    -> {field: (grad, grad_abs, grad_cnt)} over FIELDS, N-row arrays in dt (grad_cnt int64, per row)."""
    N = int(c["N"])
    ch, pa, t, live = rows(c)
    t = t.astype(dt)
    u = dt(1) - t
    raw = [np.asarray(c[k]).astype(dt) for k in FIELDS]
    arrs = activate(c, act, dt)
    sgn = np.where(_dot(arrs[2][ch], arrs[2][pa]) < 0, dt(-1), dt(1))
    cnt = np.zeros(N, np.int64)
    np.add.at(cnt, ch, 1)
    np.add.at(cnt, pa[live], 1)
    res = {}
    for k, (field, name) in enumerate(zip(FIELDS, OUTS)):
        shape = raw[k].shape
        g = np.zeros((len(ch),) + shape[1:], dt) if ups[k] is None else np.asarray(ups[k]).astype(dt)
        gc = _bc(np.where(live, t, dt(1)), g) * g  # a copy row hands its upstream on unchanged
        gp = _bc(u, g) * g
        if field == "rotation":
            gp = gp * sgn[:, None]
        terms = []
        for idx, gg in ((ch, gc), (pa[live], gp[live])):
            x = raw[k][idx]
            if act == 0 or field in ("xyz", "features"):
                terms.append((idx, gg, np.abs(gg)))
            elif field == "scaling":
                e = np.exp(x)
                terms.append((idx, gg * e, np.abs(gg * e)))
            elif field == "rotation":
                v, size = _normalize_grad(x, gg, dt)
                terms.append((idx, v, size))
            elif act == ABS:
                terms.append((idx, np.where(x > 0, gg, np.where(x < 0, -gg, dt(0))), np.abs(gg)))
            else:
                with np.errstate(over="ignore"):
                    y = dt(1) / (dt(1) + np.exp(-x))
                terms.append((idx, gg * (dt(1) - y) * y, np.abs(gg) * y * ((dt(1) - y) + np.abs(dt(1) - dt(2) * y))))
        val, size = np.zeros(shape, dt), np.zeros(shape, dt)
        for idx, v, s in terms:
            np.add.at(val, idx, v)
            np.add.at(size, idx, s)
        res[field] = (val, size, cnt)
    return res


def grad_bar(res, field):
    """(grad_cnt + 2) * 2^-24 * grad_abs per element (float64)."""
    _, size, cnt = res[field]
    return (_bc(cnt, size) + 2) * U * size.astype(np.float64)


def meets_unique_precondition(c):
    """GSR_CUT_UNIQUE_CHILDREN: no row rendered twice, no rendered row a parent (a root's row N - 1
    counts only where its weight is not 1), no rendered row a skybox row."""
    N, S = int(c["N"]), int(c["S"])
    ri = np.asarray(c["ri"], np.int64)
    pi = np.asarray(c["pi"], np.int64)[:len(ri)]
    w = np.asarray(c["w"], np.float32)[:len(ri)]
    par = np.where(pi < 0, pi + N, pi)[(pi >= 0) | (w != 1)]
    if len(np.unique(ri)) != len(ri) or np.intersect1d(ri, par).size or (len(ri) and ri.max() >= N - S):
        return False
    return not (S > 0 and (par >= N - S).any())


# ---- the blend weight (csrc/lod.hip's header) -----------------------------------------------------

FLT_MAX = float(np.finfo(np.float32).max)


def node_size(box, v):
    """size / distance of the box from the viewpoint; FLT_MAX when the viewpoint is inside (faces
    included).  float64 over float32 inputs."""
    lo, size, hi = box[0, :3].astype(np.float64), float(box[0, 3]), box[1, :3].astype(np.float64)
    v = np.asarray(v, np.float32).astype(np.float64)
    if np.all((v >= lo) & (v <= hi)):
        return FLT_MAX
    return size / float(np.sqrt(((v - np.clip(v, lo, hi)) ** 2).sum()))


def interpolation_weights(node_indices, target, nodes, boxes, v):
    """t = 1 for a root or a parent larger than 2 target; else, with s0 = max(sp / 2, s) and sp > s0,
    t = max(1 - max(0, target - s0) / (sp - s0), 0); num_kids = the parent's child count (1 for roots).
    -> (weights float64, num_kids, exact): exact[i] says every intermediate of node i is a float32
    number, so a float32 evaluation takes the same decisions and gives the same weight."""
    target = float(np.float32(target))
    f32 = lambda x: np.isinf(x) or float(np.float32(x)) == x
    w, kids, exact = [], [], []
    for i in np.asarray(node_indices):
        p = int(nodes[i, 1])
        t, k, vals = 1.0, 1, []
        if p >= 0:
            k = int(nodes[p, 6])
            sp = node_size(boxes[p], v)
            vals += [sp, 2 * target]
            if not sp > 2 * target:
                s = node_size(boxes[i], v)
                s0 = max(0.5 * sp, s)
                diff = sp - s0
                vals += [s]  # sp - s0 rounds to a float32 of the same sign: only a positive one is used
                if diff > 0:
                    vals += [diff]
                    tdiff = max(0.0, target - s0)
                    t = max(1.0 - tdiff / diff, 0.0)
                    vals += [tdiff, tdiff / diff, t]
        w.append(t)
        kids.append(k)
        exact.append(all(f32(x) for x in vals))
    return np.array(w), np.array(kids, np.int32), np.array(exact, bool)
