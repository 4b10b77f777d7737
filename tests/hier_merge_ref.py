"""numpy restatement of the hierarchy merger's rule (DESIGN.md "Hierarchy merger", rules A-E), the
checker of csrc/hier_merge.hip -- test infrastructure, as tests/hier_build_ref.py is for the builder,
whose morton_keys, topology and merge_step it reuses for the top tree.  The rule is this project's
definition (the published method's consolidation restated; parity unpinned against the un-vendored
gaussianhierarchy tool).  Ownership is evaluated in float32 exactly as the rule states it; survival,
splicing and the layout are integer; the new top rows are float64, with merge_step(..., np.float32) the
basis of the GPU test's tolerances.  Also the test problems shared by the CPU and the GPU tests.
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hier_build_ref as R  # noqa: E402

CENTRE_BATCH = 256  # the ownership kernel's LDS batch (GSR_HIER_MERGE_CENTRE_BATCH)


# ---- A. ownership --------------------------------------------------------------------------------

def owners(xyz, centres):
    """The owning chunk of fp32 positions (K,3): the first chunk, in index order, with the smallest
    d2 = (dx dx + dy dy) + dz dz, every operation rounded to fp32; -1 when no d2 is finite."""
    x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
    best = np.full(x.shape[0], np.inf, np.float32)
    owner = np.full(x.shape[0], -1, np.int64)
    with np.errstate(all="ignore"):
        for k in range(c.shape[0]):
            d = x - c[k]  # fp32
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            win = d2 < best  # false for NaN and +inf
            best[win] = d2[win]
            owner[win] = k
    return owner


# ---- B. survival and splicing --------------------------------------------------------------------

def validate(nodes):
    """The first node of (N,7) `nodes` that breaks the builder's layout, or -1."""
    nd = np.asarray(nodes, np.int64)
    N = nd.shape[0]
    for n in range(N):
        d, p, start, cl, cm, fc, cc = nd[n]
        ok = start == n
        if n == 0:
            ok &= d == 0 and p == -1
        else:
            ok &= 0 <= p < n and nd[p, 6] == 2 and nd[p, 5] in (n, n - 1) and d == nd[p, 0] + 1 and d >= nd[n - 1, 0]
        if (cl, cm, fc, cc) != (1, 0, -1, 0):
            ok &= (cl, cm, cc) == (0, 1, 2) and n < fc and fc + 1 < N
            ok = ok and nd[fc, 1] == n and nd[fc + 1, 1] == n
        if not ok:
            return n
    return -1


def splice(nodes, leaf_survives):
    """Rule B on one chunk.  leaf_survives: bool per node (read at the leaves).  Returns surv, kind
    (0 not retained, 1 retained leaf, 2 retained interior node), eff (the retained node at or below
    a surviving node: down through the nodes with one surviving child, -1 elsewhere)."""
    nd = np.asarray(nodes, np.int64)
    N = nd.shape[0]
    leaf = nd[:, 6] == 0
    surv = leaf & np.asarray(leaf_survives, bool)
    depth = nd[:, 0]
    order = [np.nonzero(depth == d)[0] for d in range(int(depth.max()) + 1)]
    for lv in order[:0:-1]:  # children before parents
        surv[nd[lv[surv[lv]], 1]] = True
    fc = np.where(leaf, 0, nd[:, 5])
    both = ~leaf & surv[fc] & surv[np.minimum(fc + 1, N - 1)]
    kind = np.where(leaf & surv, 1, np.where(both, 2, 0))
    eff = np.full(N, -1, np.int64)
    for lv in order[::-1]:
        s = lv[surv[lv]]
        kept = kind[s] > 0
        eff[s[kept]] = s[kept]
        one = s[~kept]
        eff[one] = np.where(surv[fc[one]], eff[fc[one]], eff[fc[one] + 1])
    return surv, kind, eff


# ---- C-E. the merge ------------------------------------------------------------------------------

def _rows(chunk, idx, M):
    """float64 child-row dict (hier_build_ref.merge_step's format) of a chunk's rows, |opacity|, SH padded to M."""
    n = len(idx)
    shs = np.zeros((n, M, 3))
    s = np.asarray(chunk["shs"])[idx]
    shs[:, :s.shape[1]] = s
    return dict(xyz=np.asarray(chunk["means3D"], np.float64)[idx], log_scales=np.asarray(chunk["log_scales"], np.float64)[idx],
                rotations=np.asarray(chunk["rotations"], np.float64)[idx],
                opacities=np.abs(np.asarray(chunk["opacities"], np.float64).reshape(-1)[idx]), shs=shs.reshape(n, 3 * M))


def merge(chunks, centres):
    """chunks: dicts of nodes (N_c,7), means3D, log_scales, rotations, opacities, shs (.., M_c, 3), boxes
    (N_c,2,4) (rows past N_c ignored); centres (C,3).  Returns nodes (N,7) int32, source (N,2) int32,
    leaf_rows (N), K_c, levels (all exact), boxes (N,2,4) float32 (exact: copies and fp32 unions) and the
    N rows in float64 (retained rows are the chunk's values, new top rows the float64 rule E of the
    reference's own children)."""
    C = len(chunks)
    M = max(np.asarray(c["shs"]).shape[1] for c in chunks)
    Ns = [np.asarray(c["nodes"]).shape[0] for c in chunks]
    first = np.concatenate([[0], np.cumsum(Ns)]).astype(np.int64)
    T = int(first[-1])
    for c, ch in enumerate(chunks):
        bad = validate(ch["nodes"])
        if bad >= 0:
            raise ValueError(f"chunk {c}: node {bad} breaks the hierarchy layout")
    inner_u, kids_u, K_c, roots = np.zeros(T, bool), np.zeros((T, 2), np.int64), [], []
    for c, ch in enumerate(chunks):
        nd = np.asarray(ch["nodes"], np.int64)
        N = Ns[c]
        own = owners(np.asarray(ch["means3D"], np.float32)[:N], centres)
        surv, kind, eff = splice(nd, own == c)
        K_c.append(int((kind == 1).sum()))
        roots.append(int(first[c] + eff[0]) if surv[0] else -1)
        two = np.nonzero(kind == 2)[0]
        inner_u[first[c] + two] = True
        x, y = eff[nd[two, 5]], eff[nd[two, 5] + 1]
        kids_u[first[c] + two, 0] = first[c] + np.minimum(x, y)  # child order: lower old id first
        kids_u[first[c] + two, 1] = first[c] + np.maximum(x, y)
    K = sum(K_c)
    if K == 0:
        raise ValueError("no chunk has a surviving leaf")
    active = [c for c in range(C) if K_c[c] > 0]
    Ca = len(active)
    chunk_of = np.searchsorted(first, np.arange(T), side="right") - 1

    # C. top tree over the active chunks' root rows
    Nt = 2 * Ca - 1
    top = {k: np.zeros((Nt,) + s) for k, s in (("xyz", (3,)), ("log_scales", (3,)), ("rotations", (4,)),
                                                ("opacities", ()), ("shs", (3 * M,)))}
    tbox = np.zeros((Nt, 2, 4), np.float32)
    tnodes = np.zeros((1, 7), np.int32)
    tleaf = np.zeros(1, np.int32)
    if Ca > 1:
        rxyz = np.stack([np.asarray(chunks[c]["means3D"], np.float32)[roots[c] - first[c]] for c in active])
        tnodes, tleaf, tlevels = R.topology(R.morton_keys(rxyz))
        for t in np.nonzero(tleaf >= 0)[0]:
            c = active[tleaf[t]]
            row = _rows(chunks[c], [roots[c] - first[c]], M)
            for k in top:
                top[k][t] = row[k][0]
            tbox[t] = np.asarray(chunks[c]["boxes"], np.float32)[roots[c] - first[c]]
        for d in range(tlevels - 2, -1, -1):
            idx = np.nonzero((tnodes[:, 0] == d) & (tnodes[:, 6] == 2))[0]
            ca = tnodes[idx, 5]
            a, b = {k: v[ca] for k, v in top.items()}, {k: v[ca + 1] for k, v in top.items()}
            a["opacities"], b["opacities"] = np.abs(a["opacities"]), np.abs(b["opacities"])
            m = R.merge_step(a, b)
            for k in top:
                top[k][idx] = m[k]
            tbox[idx, 0, :3] = np.minimum(tbox[ca, 0, :3], tbox[ca + 1, 0, :3])
            tbox[idx, 1, :3] = np.maximum(tbox[ca, 1, :3], tbox[ca + 1, 1, :3])
            tbox[idx, 0, 3] = R.box_extent(tbox[idx])
            tbox[idx, 1, 3] = 0

    # D. layout: ids of the joined topology -- input node g -> g, top node t -> T + t; a top leaf is its chunk's root
    def top_id(t):
        return np.where(tleaf[t] >= 0, np.asarray([roots[active[l]] if l >= 0 else -1 for l in tleaf[t]]), T + t)

    N = 2 * K - 1
    nodes = np.zeros((N, 7), np.int32)
    ids = np.zeros(N, np.int64)
    ids[0] = T if Ca > 1 else roots[active[0]]
    nodes[0, :2] = (0, -1)
    s, e, depth = 0, 1, 0
    while True:
        lv = ids[s:e]
        is_top = lv >= T
        inner = np.where(is_top, tnodes[np.where(is_top, lv - T, 0), 6] == 2, inner_u[np.where(is_top, 0, lv)])
        n_in = np.nonzero(inner)[0] + s
        c0 = e + 2 * np.arange(len(n_in))
        nodes[s:e, 2] = np.arange(s, e)
        nodes[s:e, 3], nodes[s:e, 4] = ~inner, inner
        nodes[s:e, 5], nodes[s:e, 6] = -1, 0
        nodes[n_in, 5], nodes[n_in, 6] = c0, 2
        if not len(n_in):
            break
        pid = ids[n_in]
        kids = kids_u[np.where(pid >= T, 0, pid)]
        tp = pid >= T
        if tp.any():
            a = tnodes[pid[tp] - T, 5].astype(np.int64)
            kids[tp, 0], kids[tp, 1] = top_id(a), top_id(a + 1)
        ids[c0], ids[c0 + 1] = kids[:, 0], kids[:, 1]
        for k in (c0, c0 + 1):
            nodes[k, 0], nodes[k, 1] = depth + 1, n_in
        s, e, depth = e, e + 2 * len(n_in), depth + 1
    assert e == N
    is_top = ids >= T
    g = np.where(is_top, 0, ids)
    source = np.stack([np.where(is_top, -1, chunk_of[g]), np.where(is_top, -1, g - first[chunk_of[g]])], 1).astype(np.int32)
    leaf_rows = np.where(nodes[:, 6] == 0, source[:, 1], -1).astype(np.int32)

    # E. rows
    out = dict(means3D=np.zeros((N, 3)), log_scales=np.zeros((N, 3)), rotations=np.zeros((N, 4)), opacities=np.zeros(N),
               shs=np.zeros((N, M, 3)))
    boxes = np.zeros((N, 2, 4), np.float32)
    for c in active:
        sel = np.nonzero(source[:, 0] == c)[0]
        old = source[sel, 1]
        ch = chunks[c]
        out["means3D"][sel], out["log_scales"][sel] = np.asarray(ch["means3D"])[old], np.asarray(ch["log_scales"])[old]
        out["rotations"][sel], out["opacities"][sel] = np.asarray(ch["rotations"])[old], np.asarray(ch["opacities"]).reshape(-1)[old]
        sh = np.asarray(ch["shs"])[old]
        out["shs"][sel, :sh.shape[1]] = sh
        boxes[sel] = np.asarray(ch["boxes"], np.float32)[old]
    tsel = np.nonzero(is_top)[0]
    t = ids[tsel] - T
    out["means3D"][tsel], out["log_scales"][tsel], out["rotations"][tsel] = top["xyz"][t], top["log_scales"][t], top["rotations"][t]
    out["opacities"][tsel], out["shs"][tsel] = top["opacities"][t], top["shs"][t].reshape(-1, M, 3)
    boxes[tsel] = tbox[t]
    return dict(nodes=nodes, source=source, leaf_rows=leaf_rows, K_c=K_c, levels=depth + 1, boxes=boxes, **out)


def top_children(h):
    """The new top nodes of merged arrays `h` (the reference's dict or the device's arrays as numpy) and
    their two child rows as merge_step takes them: fp32 rows, |opacity|."""
    nodes, src = np.asarray(h["nodes"]), np.asarray(h["source"])
    N = nodes.shape[0]
    idx = np.nonzero(src[:, 0] < 0)[0]
    ca = nodes[idx, 5]
    f = lambda x: np.asarray(x, np.float32)
    rows = dict(xyz=f(h["means3D"]).reshape(N, 3), log_scales=f(h["log_scales"]).reshape(N, 3),
                rotations=f(h["rotations"]).reshape(N, 4), opacities=f(h["opacities"]).reshape(N), shs=f(h["shs"]).reshape(N, -1))
    pick = lambda k: {n: (np.abs(v[k]) if n == "opacities" else v[k]) for n, v in rows.items()}
    return idx, pick(ca), pick(ca + 1), {n: v[idx] for n, v in rows.items()}


# ---- the test problems (shared by the CPU and the GPU tests) ------------------------------------------

def perturb(h, seed):
    """A built chunk hierarchy (numpy arrays, hier_build_ref.build's keys) with its attributes moved as
    train_post moves them -- every row, interior ones included -- and every seventh opacity negative (the
    loader of a trained hierarchy takes |o|).  nodes and boxes stay.  fp32 arrays, opacities (N,1)."""
    rng = np.random.default_rng(seed)
    N = np.asarray(h["nodes"]).shape[0]
    f = lambda x: np.ascontiguousarray(x, np.float32)
    op = np.asarray(h["opacities"], np.float64).reshape(N) * rng.uniform(0.8, 1.2, N)
    op[::7] *= -1.0
    return dict(nodes=np.ascontiguousarray(h["nodes"], np.int32), boxes=f(h["boxes"]),
                means3D=f(np.asarray(h["means3D"]) + rng.normal(0, 0.01, (N, 3))),
                log_scales=f(np.asarray(h["log_scales"]) + rng.normal(0, 0.05, (N, 3))),
                rotations=f(np.asarray(h["rotations"]) + rng.normal(0, 0.02, (N, 4))), opacities=f(op).reshape(N, 1),
                shs=f(np.asarray(h["shs"]) + rng.normal(0, 0.01, np.asarray(h["shs"]).shape)))


def _grid_centres(C, pitch):
    i = np.arange(C)
    return np.stack([(i % 10) * pitch, (i // 10) * pitch, np.full(C, 10.0)], 1).astype(np.float32)


# name -> (the chunks' (P, M) list, centres (C,3), each chunk's cloud offset (C,3) or None).  Every cloud
# is hier_build_ref.cloud("random", P, M, seed): x, y within about +-10, z in 2..20.
def case(name):
    z3 = lambda C: np.zeros((C, 3), np.float32)
    if name == "c1_p1":
        return [(1, 16)], np.array([[0, 0, 10]], np.float32), None
    if name == "c1_p1000":  # everything is owned: the output equals the input
        return [(1000, 4)], np.array([[3, -2, 5]], np.float32), None
    if name == "c2_p64_p65":  # two overlapping clouds cut by the plane x = 0
        return [(64, 16), (65, 16)], np.array([[-1, 0, 10], [1, 0, 10]], np.float32), None
    if name == "c2_slab":  # the bisector is z = 3: chunk 0 keeps a thin slab of its cloud, long splice chains
        return [(1000, 4), (1000, 4)], np.array([[0, 0, -100], [0, 0, 106]], np.float32), None
    if name == "c2_equidistant":  # with_ties() puts leaves on the bisector x = 0
        return [(200, 4), (200, 4)], np.array([[-1, 0, 10], [1, 0, 10]], np.float32), None
    if name == "c2_one_empty":  # chunk 1's centre is farther from every leaf
        return [(300, 4), (300, 4)], np.array([[0, 0, 10], [0, 0, 1000]], np.float32), None
    if name == "c3_mixed":  # SH widths differ; a one-leaf chunk, moved to where it owns itself
        return [(4097, 16), (3000, 4), (1, 16)], np.array([[-3, 0, 10], [3, 0, 10], [0, 40, 10]], np.float32), \
            np.array([[0, 0, 0], [0, 0, 0], [0, 40, 0]], np.float32)
    if name == "c70_p300":  # the top tree has several levels and straddles a wave
        cen = _grid_centres(70, 8.0)
        return [(300, 4)] * 70, cen, cen * np.array([1, 1, 0], np.float32)
    if name == "c_batch_plus_1":  # one more chunk than the ownership kernel's centre batch
        cen = _grid_centres(CENTRE_BATCH + 1, 30.0)
        return [(3, 4)] * (CENTRE_BATCH + 1), cen, cen * np.array([1, 1, 0], np.float32)
    if name == "c4_p20000":  # crosses every workgroup and tile limit
        cen = np.array([[-4, -2, 10], [4, -2, 10], [-4, 2, 10], [4, 2, 10]], np.float32)
        return [(20000, 16)] * 4, cen, z3(4)
    if name == "nan_leaves":
        return [(300, 4), (300, 4)], np.array([[-1, 0, 10], [1, 0, 10]], np.float32), None
    if name == "all_nonfinite":
        return [(5, 4), (5, 4)], np.array([[-1, 0, 10], [1, 0, 10]], np.float32), None
    raise ValueError(name)


CASES = ["c1_p1", "c1_p1000", "c2_p64_p65", "c2_slab", "c2_equidistant", "c2_one_empty", "c3_mixed", "c70_p300",
         "c_batch_plus_1", "c4_p20000", "nan_leaves"]


def case_clouds(name):
    """The builder inputs of a case: one cloud dict per chunk (seed = 1000 chunk + P), and the centres."""
    spec, centres, offs = case(name)
    clouds = []
    for c, (P, M) in enumerate(spec):
        cl = R.cloud("random", P, M, seed=1000 * c + P)
        if offs is not None:
            cl["xyz"] = (cl["xyz"] + offs[c]).astype(np.float32)
        clouds.append(cl)
    return clouds, centres


def finish_case(name, built):
    """The case's chunk hierarchies from `built`, the builder's output per chunk (numpy arrays): perturbed
    as train_post would, then the case's own edits of the leaves' means."""
    chunks = [perturb(h, seed=17 * c + 1) for c, h in enumerate(built)]
    for c, ch in enumerate(chunks):
        leaves = np.nonzero(ch["nodes"][:, 6] == 0)[0]
        if name == "c1_p1000":
            pass
        elif name == "c2_equidistant":
            ch["means3D"][leaves[::5], 0] = 0.0  # d2 to (-1,0,10) and (1,0,10) is bitwise the same
        elif name == "nan_leaves":
            ch["means3D"][leaves[::9], 1] = np.nan
            ch["means3D"][leaves[4::9], 2] = np.inf
        elif name == "all_nonfinite":
            ch["means3D"][leaves[::2]] = np.nan
            ch["means3D"][leaves[1::2], 0] = -np.inf
    return chunks


def cpu_case(name, _cache={}):
    """A case with its chunks built by hier_build_ref.build on the CPU (small cases): chunks, centres."""
    if name not in _cache:
        clouds, centres = case_clouds(name)
        _cache[name] = (finish_case(name, [R.build(**cl) for cl in clouds]), centres)
    return _cache[name]


# the cut checks of the CPU and the GPU tests: three viewpoints, three targets each
VIEWPOINTS = [(0.0, 0.0, -50.0), (40.0, 10.0, 8.0), (-3.0, 1.0, 9.0)]  # outside, beside and inside the clouds
TARGET_FRACTIONS = (0.3, 0.05, 0.0)  # of the root's extent over its distance


def targets(boxes, v):
    """The three cut targets of a viewpoint: fractions of the root box's size over its distance (fp32)."""
    c = 0.5 * (boxes[0, 0, :3] + boxes[0, 1, :3])
    d = max(float(np.linalg.norm(c - np.asarray(v, np.float32))), 1.0)
    return [np.float32(float(boxes[0, 0, 3]) / d * f) for f in TARGET_FRACTIONS]


def assert_cut_covers_each_leaf_once(nodes, ni):
    """Every leaf has exactly one ancestor-or-self among the rendered nodes ni, and nothing else is rendered."""
    N = nodes.shape[0]
    assert len(np.unique(ni)) == len(ni) and (ni >= 0).all() and (ni < N).all()
    cover = np.zeros(N, np.int64)
    cover[ni] = 1
    for n in range(1, N):  # parents are stored before their children
        cover[n] += cover[nodes[n, 1]]
    assert (cover[nodes[:, 6] == 0] == 1).all()


def fp32_basis(cases=CASES, chunks_of=cpu_case):
    """The basis of the GPU test's tolerances: the largest error a float32 numpy evaluation of rule E
    shows against float64 on the cases' own top-tree steps -- every new top node's two child rows of the
    reference's merge, rounded to fp32 as a device holds them, |opacity|."""
    worst = dict(mu=0.0, sh=0.0, opacity=0.0, cov=0.0)
    for name in cases:
        chunks, centres = chunks_of(name)
        idx, a, b, _ = top_children(merge(chunks, centres))
        if not len(idx):
            continue
        e = R.step_errors(R.merge_step(a, b, np.float32), R.merge_step(a, b), a, b)
        worst = {k: max(v, e[k]) for k, v in worst.items()}
    return worst


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "street-sparse-3dgs_amd"))
    for k, v in fp32_basis().items():
        print(f"{k}: measured {v:.3e}  bound (4x) {4 * v:.3e}")
