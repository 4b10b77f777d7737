"""numpy float64 reference of densify-and-prune: scene/gaussian_model.py:672-778 (densify_and_clone,
densify_and_split, the opacity prune, optionally compare_points_to_gt) restated as one function over
the old rows, for tests/test_gpu_densify_edges.py and tests/test_densify_cases_cpu.py.  first_row
stands for scaffold_points.  Importable without a GPU and without torch.

Decision quantities, per old row i (o, s, g, r the float32 inputs read as float64):

    op    = 1 / (1 + exp(-o))                               torch.sigmoid
    c     = g * r * op ** 0.2        (g = 0 where NaN)      the split's quantity; the clone's uses |g|
    smax  = max_j exp(s_j)
    eligible = i >= first_row and op > float32(0.15)
    clone = eligible and |g| r op^0.2 >= max_grad and smax <= max_scale
    split = eligible and  g  r op^0.2 >= max_grad and smax >  max_scale
    prune = i >= first_row and op < min_opacity

max_grad, min_opacity and max_scale = percent_dense * extent are rounded to float32 first, as the C
ABI (and torch, comparing a float32 tensor with a Python scalar) receives them; everything else is
float64.  A NaN quantity compares false.  The reference clones first, then splits (drawing both
children's samples for every split row, pruned or not), then prunes by opacity: the output is the
kept old rows, the kept clones, the first children, the second children, each in source order; a
clone or a child shares its source's opacity and goes with it.

undecided() names the rows whose decision an fp32 evaluation may legitimately take the other way.
UNDECIDED_REL = 2^-18 relative to the threshold: densify_flags_kernel's chain to c is expf (1 ulp),
an add, a divide (both correctly rounded), powf (1 ulp of its own, and 0.2 of op's error; its
exponent float32(0.2) moves the result by under 0.1 ulp for op >= 0.15), sqrtf(g * g) (two
roundings) and two multiplies -- under 8 ulps = 16 * 2^-24 = 2^-20 relative; op and exp(s_j) alone
carry less.  2^-18 is four times that.
"""
from __future__ import annotations

import numpy as np

import gt_ref

KIND_OLD, KIND_CLONE, KIND_CHILD1, KIND_CHILD2 = 0, 1, 2, 3
PARAMS = ("xyz", "features", "opacity", "scaling", "rotation")
WIDTHS = {"xyz": 3, "features": 48, "opacity": 1, "scaling": 3, "rotation": 4}
UNDECIDED_REL = 2.0 ** -18
OP_ELIGIBLE = float(np.float32(0.15))
LN_1_6 = float(np.log(1.6))


def thresholds(max_grad, min_opacity, extent, percent_dense):
    """The scalars as the kernels receive them (float32), as Python floats."""
    return dict(max_grad=float(np.float32(max_grad)), min_op=float(np.float32(min_opacity)),
                max_scale=float(np.float32(float(percent_dense) * float(extent))))


def quantities(opacity, scaling, accum, max_radii):
    """op, the clone's and the split's gradient quantity, smax: float64, one per row."""
    o = np.asarray(opacity, np.float64).reshape(-1)
    s = np.asarray(scaling, np.float64).reshape(-1, 3)
    g = np.asarray(accum, np.float64).reshape(-1).copy()
    r = np.asarray(max_radii, np.float64).reshape(-1)
    g[np.isnan(g)] = 0.0  # grads[grads.isnan()] = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        op = 1.0 / (1.0 + np.exp(-o))
        pw = op ** 0.2
        c_split = g * r * pw
        c_clone = np.abs(g) * r * pw  # torch.norm(grads, dim=-1) of a (P, 1) tensor
        smax = np.exp(s).max(axis=1) if s.shape[0] else np.zeros(0)
    return op, c_clone, c_split, smax


def predicates(opacity, scaling, accum, max_radii, max_grad, min_opacity, extent, percent_dense, first_row=0):
    """(clone, split, prune) per old row, by the reference source's comparison operators."""
    t = thresholds(max_grad, min_opacity, extent, percent_dense)
    op, c_clone, c_split, smax = quantities(opacity, scaling, accum, max_radii)
    movable = np.arange(op.shape[0]) >= int(first_row)
    with np.errstate(invalid="ignore"):
        eligible = movable & (op > OP_ELIGIBLE)
        clone = eligible & (c_clone >= t["max_grad"]) & (smax <= t["max_scale"])
        split = eligible & (c_split >= t["max_grad"]) & (smax > t["max_scale"])
        prune = movable & (op < t["min_op"])
    return clone, split, prune


def undecided(opacity, scaling, accum, max_radii, max_grad, min_opacity, extent, percent_dense, first_row=0,
              exact_ties=()):
    """Rows (sorted indices) with a decision quantity within UNDECIDED_REL of its threshold, the
    constructed exact ties excepted (their quantities are exact in fp32 by construction)."""
    t = thresholds(max_grad, min_opacity, extent, percent_dense)
    op, c_clone, c_split, smax = quantities(opacity, scaling, accum, max_radii)

    def near(q, thr):
        with np.errstate(invalid="ignore"):
            return np.abs(q - thr) <= UNDECIDED_REL * abs(thr)  # NaN and Inf: False

    bad = near(op, OP_ELIGIBLE) | near(op, t["min_op"]) | near(smax, t["max_scale"]) | \
        near(c_clone, t["max_grad"]) | near(c_split, t["max_grad"])
    bad[np.asarray(list(exact_ties), np.int64)] = False
    return np.nonzero(bad)[0]


def rotation(q):
    """utils/general_utils.py build_rotation: (n, 3, 3) of q / |q| in float64 (NaN for a zero q)."""
    q = np.asarray(q, np.float64).reshape(-1, 4)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    r, x, y, z = n[:, 0], n[:, 1], n[:, 2], n[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)
    return R


def plan(params, accum, max_radii, max_grad, min_opacity, extent, percent_dense, first_row=0, cloud=None, thr=None):
    """The row map and the counts.  With a cloud (float32 (G, 3)) and thr: rows inside its XY bounds
    with no cloud point within thr (tests/gt_ref.far_mask, float32-exact) lose their old row and
    their clone -- rows below first_row too; split and opacity-pruned rows are not tested."""
    clone, split, prune = predicates(params["opacity"], params["scaling"], accum, max_radii, max_grad, min_opacity,
                                     extent, percent_dense, first_row)
    P0 = clone.shape[0]
    keep_old, keep_clone, keep_split = ~split & ~prune, clone & ~prune, split & ~prune
    out = {}
    if cloud is not None:
        far = gt_ref.far_mask(np.asarray(params["xyz"], np.float32).reshape(-1, 3), cloud, thr, skip=split | prune) \
            if P0 else np.zeros(0, bool)
        out["gt_pruned"] = int((keep_old & far).sum() + (keep_clone & far).sum())
        out["gt_pruned_fixed"] = int((keep_old & far)[:int(first_row)].sum())
        out["far"] = far
        keep_old, keep_clone = keep_old & ~far, keep_clone & ~far
    rank_all = np.cumsum(split) - split  # counted over every split row: samples are drawn before the prune
    i_old, i_clone, i_split = np.nonzero(keep_old)[0], np.nonzero(keep_clone)[0], np.nonzero(keep_split)[0]
    src = np.concatenate([i_old, i_clone, i_split, i_split]).astype(np.int64)
    kind = np.concatenate([np.full(i_old.size, KIND_OLD), np.full(i_clone.size, KIND_CLONE),
                           np.full(i_split.size, KIND_CHILD1), np.full(i_split.size, KIND_CHILD2)]).astype(np.int64)
    rank = np.concatenate([np.zeros(i_old.size + i_clone.size, np.int64), rank_all[i_split], rank_all[i_split]])
    out.update(src=src, kind=kind, rank=rank.astype(np.int64), clone=clone, split=split, prune=prune,
               counts=dict(kept=int(i_old.size), cloned=int(i_clone.size), split=int(split.sum()),
                           total=int(src.size)), split_kept=int(i_split.size))
    return out


def densify_ref(params, moments, accum, max_radii, normals, max_grad, min_opacity, extent, percent_dense,
                first_row=0, cloud=None, thr=None):
    """params: {name: (P0, ...) float32} for PARAMS; moments: {name: (exp_avg, exp_avg_sq)} for the
    parameters that have Adam state; normals: (2 n_split, 3) standard-normal draws, n_split counted
    over all split rows.  Returns plan()'s dict plus params / moments ({name: float64 arrays of
    `total` rows}), child_bound_xyz / child_bound_scaling (see child_bounds) and stats_rows."""
    out = plan(params, accum, max_radii, max_grad, min_opacity, extent, percent_dense, first_row, cloud, thr)
    src, kind, rank = out["src"], out["kind"], out["rank"]
    n_split = out["counts"]["split"]
    z = np.asarray(normals, np.float64).reshape(-1, 3)
    assert z.shape[0] == 2 * n_split, (z.shape, n_split)
    new = {}
    for name in PARAMS:
        a = np.asarray(params[name])
        new[name] = a.astype(np.float64)[src]  # old rows and clones: copies
    child = kind >= KIND_CHILD1
    cs = src[child]
    zr = np.where(kind[child] == KIND_CHILD1, 0, n_split) + rank[child]
    s = np.asarray(params["scaling"], np.float64).reshape(-1, 3)[cs]
    with np.errstate(invalid="ignore", over="ignore"):
        samples = z[zr] * np.exp(s)
        R = rotation(np.asarray(params["rotation"]).reshape(-1, 4)[cs])
        xyz = np.asarray(params["xyz"], np.float64).reshape(-1, 3)[cs]
        new["xyz"][child] = np.einsum("nij,nj->ni", R, samples) + xyz
        new["scaling"][child] = s - LN_1_6  # log(exp(s) / (0.8 * 2))
    mom = {}
    for name, (m, v) in moments.items():
        mm, vv = np.asarray(m).astype(np.float64)[src], np.asarray(v).astype(np.float64)[src]
        mm[kind != KIND_OLD] = 0.0  # cat_tensors_to_optimizer: zeros for every new row
        vv[kind != KIND_OLD] = 0.0
        mom[name] = (mm, vv)
    bx, bs = child_bounds(xyz, np.abs(samples).sum(axis=1), new["scaling"][child])
    out.update(params=new, moments=mom, child=child, child_bound_xyz=bx, child_bound_scaling=bs)
    return out


# ---- how far a correct fp32 evaluation of a split child may lie from the float64 one -------------
# u = 2^-24 is fp32's unit roundoff; expf, logf: 1 ulp <= 2u relative; +, *, /, sqrtf, fmaf: u.
#
# xyz_c = fma(R_c2, t_2, fma(R_c1, t_1, R_c0 * t_0)) + xyz_c,  t_j = z_j * expf(s_j)
#   t_j:        expf 2u, the product u                                          -> 3u |t_j|
#   |q|:        four squares (u each) and three adds (u each) of positive terms: the sum within 4u,
#               its root within 2u, sqrtf's own u                               -> 3u
#   r, x, y, z: q_k / |q|: 3u and the divide's u                                -> 4u, each <= 1
#   R diagonal  1 - 2 (y y + z z): y y within 2 * 4u + u = 9u, the sum's u: 10u (y y + z z) <= 10u,
#               doubled 20u, the subtraction's u |R_cc| <= u                    -> 21u absolute
#   R off-diag  2 (x y -+ r z): products within 9u, |x y| + |r z| <= 1/2, the sum's u / 2, doubled
#                                                                               -> 10u absolute
#   The entries' errors are absolute (cancellation against 1), so they weigh on |t_j|, not on
#   |R_cj t_j|: sum_j 21u |t_j|.  The products carry t_j's 3u (|R_cj| <= 1), the product and the
#   two fmaf another 3u, the final add u of the result:
#       |got - ref| <= (21 + 3 + 3 + 1) u sum_j |t_j| + u |xyz_c|  <=  28 u (|xyz_c| + sum_j |t_j|)
#   K_XYZ = 32 leaves the second-order terms (28u * 3u and the like) and the float64 side's own
#   rounding far inside.
#
# scaling' = logf(expf(s) * c),  c = fl(1 / fl(1.6)):  fl(1.6) u, the reciprocal u, expf 2u, the
#   product u: the argument is exp(s) / 1.6 within 5u relative, its logarithm within 5u absolute;
#   logf's own ulp is 2u |result|:
#       |got - (s - ln 1.6)| <= 5u + 2u |s - ln 1.6|;  K_SCALING_ABS = 6 for the second-order terms.
K_XYZ = 32.0
K_SCALING_ABS, K_SCALING_REL = 6.0, 2.0
U = 2.0 ** -24


def child_bounds(xyz, sum_abs_samples, scaling_ref):
    """(n, 3) bounds on |fp32 - float64| for the children's xyz and scaling."""
    bx = K_XYZ * U * (np.abs(xyz) + np.asarray(sum_abs_samples)[:, None])
    bs = U * (K_SCALING_ABS + K_SCALING_REL * np.abs(scaling_ref))
    return bx, bs


def stats_ref(radii, grad2d, max_r, accum, denom):
    """add_densification_stats (scene/gaussian_model.py:780-793 and train_single.py's max_radii2D
    update) in float64 with torch.max's NaN rule (np.maximum propagates NaN); rows with radii <= 0
    are untouched.  Returns float64 (max_r, accum, denom)."""
    radii = np.asarray(radii).reshape(-1)
    g = np.asarray(grad2d, np.float64).reshape(-1, 3)
    mr, acc, den = (np.asarray(a, np.float64).reshape(-1).copy() for a in (max_r, accum, denom))
    vis = radii > 0
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
        mr[vis] = np.maximum(mr[vis], radii[vis].astype(np.float64))
        acc[vis] = np.maximum(n[vis], acc[vis])
    den[vis] += 1.0
    return mr, acc, den
