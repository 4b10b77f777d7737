"""TEST INFRASTRUCTURE ONLY -- small named inputs of the hierarchy-cut blend (csrc/hier.hip) where a wrong
sign at a tie or a dropped sibling contribution trains a slightly different hierarchy without a NaN, and
hand-built hierarchies for the blend weight (csrc/lod.hip).  tests/cut_ref.py describes a case's fields.

case(name, form): form "act" holds activated values (gsr_interpolate_cut_forward), "raw" the raw
parameters (log-scales in [-20, 3], unnormalised quaternions, stored opacities) of the _act entry points.
Extra fields: unique (the case meets GSR_CUT_UNIQUE_CHILDREN's precondition), tie (R, bool: the row's
rotation dot is exactly 0 in float32 under any summation order), runs ((start, length) of every sibling
run in row order).  Every render and parent index is in [0, N) or a root's -1: the kernels do not check
them.

tests/test_cut_cases_cpu.py holds the cases to what they are for and to the condition that no row is
one a float32 evaluation could decide either way.  A quaternion of norm exactly float32(1e-12) is
left out for that reason: float32's eps is float32(1e-12) < 1e-12, so a float64 F.normalize clamps the
row that float32 does not; the cases hold norms 1e-3 relative either side of it instead.
"""
from __future__ import annotations

import functools

import numpy as np

F = np.float32
FORMS = ("act", "raw")
RUN_LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 300)
WEIGHTS = (0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5)
OPACITY_EDGES = (0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0)
QUAT_NORMS = (0.0, 1e-13, 0.999e-12, 1.001e-12, 1e-3, 1e3)


def _fields(rng, N, M, form):
    q = rng.normal(size=(N, 4))
    if form == "act":
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        sc, op = np.exp(rng.uniform(-6, 1, (N, 3))), rng.uniform(0.01, 1, (N, 1))
    else:
        q *= np.exp(rng.uniform(-2, 2, (N, 1)))
        sc, op = rng.uniform(-20, 3, (N, 3)), 3 * rng.normal(size=(N, 1))
    return dict(xyz=(10 * rng.normal(size=(N, 3))).astype(F), scaling=sc.astype(F), rotation=q.astype(F),
                opacity=op.astype(F), features=rng.normal(size=(N, M, 3)).astype(F))


def _runs_of(pi):
    """(start, length) of every maximal run of equal consecutive parents."""
    pi = np.asarray(pi)
    if not len(pi):
        return []
    cut = np.flatnonzero(np.diff(pi) != 0) + 1
    starts = np.concatenate([[0], cut])
    return list(zip(starts.tolist(), np.diff(np.concatenate([starts, [len(pi)]])).tolist()))


def _case(name, form, N, M, S, ri, pi, w, seed, unique, tie=None, edit=None):
    rng = np.random.default_rng(seed)
    c = _fields(rng, N, M, form)
    ri, pi = np.asarray(ri, np.int32), np.asarray(pi, np.int32)
    c.update(name=f"{name}/{form}", form=form, N=N, M=M, S=S, ri=ri, pi=pi, w=np.asarray(w, F), unique=unique,
             tie=np.zeros(len(ri), bool) if tie is None else np.asarray(tie, bool), runs=_runs_of(pi))
    if edit:
        edit(c, rng)
    assert len(ri) == len(pi) == len(c["w"]) and 0 <= S <= N
    assert not len(ri) or (ri.min() >= 0 and ri.max() < N and pi.min() >= -1 and pi.max() < N)
    return c


def _sibling_layout(lengths, rng, roots=()):
    """Children rows [0, R) in a random order, one parent row per run after them (-1 for the runs
    listed in roots) -> (ri, pi, rows used)."""
    R, P = int(sum(lengths)), len(lengths)
    ri = rng.permutation(R)
    parents = R + rng.permutation(P)
    if roots:
        parents[list(roots)] = -1
    return ri, np.repeat(parents, lengths), R + P


def _placed_runs():
    """Run lengths in row order such that, for every length L of RUN_LENGTHS, runs of L start or end at
    -1, 0 and +1 from a multiple of 64 (so of 16), one run of each of 17 / 64 / 65 starts next to a
    multiple of 256, and the run of 300 covers an aligned block of 256 rows.  The rows in between are
    runs of 1 to 3."""
    lengths, pos = [], 0

    def fill(to):
        nonlocal pos
        k = 0
        while pos < to:
            n = min(to - pos, 1 + k % 3)
            lengths.append(n)
            pos += n
            k += 1

    def where(L, B, off, end):
        at = pos + 1  # a filler run in between: two placed runs never merge
        while (at + (L if end else 0) - off) % B:
            at += 1
        return at

    todo = [(L, 64, off, bool((i + off) % 2)) for i, L in enumerate(RUN_LENGTHS[:-1]) for off in (-1, 0, 1)]
    todo += [(17, 256, -1, False), (64, 256, 0, False), (65, 256, 1, False), (300, 256, -22, False)]
    while todo:  # the placement that wastes the fewest rows next
        nxt = min(todo, key=lambda p: where(*p))
        todo.remove(nxt)
        fill(where(*nxt))
        lengths.append(nxt[0])
        pos += nxt[0]
    return lengths


def _layout_case(name, form, lengths, S=0, M=16, seed=0, roots=(), root_w=1.0, unique=True, spare=3):
    rng = np.random.default_rng(seed + 1000)
    ri, pi, used = _sibling_layout(lengths, rng, roots)
    w = rng.uniform(0.05, 0.95, len(ri))
    w[pi < 0] = root_w
    return _case(name, form, used + spare + S, M, S, ri, pi, w, seed, unique)


def sized_case(R, S, M=16, form="raw", spare=3, seed=0):
    """R rendered rows in sibling runs of 1 to 6 and S skybox rows; N = R + runs + spare + S."""
    rng = np.random.default_rng(seed + 7 * R + S)
    lengths = []
    while sum(lengths) < R:
        lengths.append(min(R - sum(lengths), int(rng.integers(1, 7))))
    roots = (0,) if lengths else ()
    return _layout_case(f"sized_R{R}_S{S}_M{M}_x{spare}_{seed}", form, lengths, S=S, M=M, seed=seed + R + S, roots=roots, spare=spare)


# ---- rotation ties ---------------------------------------------------------------------------------

# (child, parent, dot): every product is a dyadic number of a few bits, so the float32 dot is exact in
# any order.  Activated form: the kernel does not normalise.
ACT_PAIRS = [((1, 2, -1, .5), (2, -1, 0, 0), 0), ((1, 2, 5, 7), (2, -1, 0, 0), 0), ((0, 0, 1, 1), (2, -1, 0, 0), 0),
             ((-1, -2, 3, 3), (2, -1, 0, 0), 0), ((1, 0, 0, 0), (0, 1, 0, 0), 0), ((1, 1, 1, 1), (1, -1, 1, -1), 0),
             ((.5, .5, .5, .5), (0, 0, 0, 0), 0), ((0, 0, 0, 0), (.5, .5, -.5, .5), 0),
             ((1, 1, 1, 1), (-0., -0., -0., -0.), 0), ((1, -1, 1, -1), (0., -0., -0., 0.), 0),
             ((1, 2, -1, .5), (2, -1, 0, .5), .25), ((1, 2, -1, .5), (2, -1, 0, -.5), -.25),
             ((1, 2, -1, .5), (2, -1, -.25, 0), .25), ((1, 2, -1, .5), (2, -1, .25, 0), -.25)]
# Raw form: norms that are powers of two, so normalize is exact; the dot is of the normalised rows.  Unit
# rows with a power-of-two norm offer no dot of 0.25: the signed rows have exactly +-0.5 and +-1.
RAW_PAIRS = [((1, 1, 1, 1), (1, -1, 1, -1), 0), ((2, 0, 0, 0), (0, 2, 0, 0), 0), ((4, 4, 4, 4), (.5, -.5, .5, -.5), 0),
             ((0, 0, .25, 0), (8, 0, 0, 0), 0), ((1, 1, 1, 1), (0, 0, 0, 0), 0), ((0, 0, 0, 0), (1, 1, -1, 1), 0),
             ((-1, 1, 1, -1), (-0., -0., 0., -0.), 0),
             ((1, 1, 1, 1), (1, -1, 1, 1), .5), ((1, 1, 1, 1), (-1, 1, -1, -1), -.5),
             ((2, 0, 0, 0), (2, 0, 0, 0), 1), ((2, 0, 0, 0), (-8, 0, 0, 0), -1),
             ((1, 1, 1, 1), (0, 0, 0, 2), .5), ((1, 1, 1, 1), (0, -4, 0, 0), -.5)]
TIE_WEIGHTS = (0.0, 0.25, 0.5, 2.0 ** -24, 0.75)  # never 1: the parent's sign must reach the output


def _ties(form):
    """One row per (pair, weight), each with its own child and parent row; then, per distinct parent
    quaternion that has several tie children, one sibling run of those children under one shared parent;
    then (raw) rows whose quaternions have the norms of QUAT_NORMS, as child and as parent."""
    pairs = ACT_PAIRS if form == "act" else RAW_PAIRS
    quats, ri, pi, w, tie = [], [], [], [], []

    def row(q):
        quats.append(q)
        return len(quats) - 1

    for qc, qp, dot in pairs:
        for t in TIE_WEIGHTS:
            ri.append(row(qc))
            pi.append(row(qp))
            w.append(t)
            tie.append(dot == 0)
    shared = {}
    for qc, qp, dot in pairs:
        if dot == 0 and any(qp):
            shared.setdefault(qp, []).append(qc)
    for qp, kids in shared.items():
        p = row(qp)
        for k, qc in enumerate(kids * 3):  # a run of tie siblings, every weight
            ri.append(row(qc))
            pi.append(p)
            w.append(TIE_WEIGHTS[k % len(TIE_WEIGHTS)])
            tie.append(True)
    fixed = len(quats)
    n_norm = 0
    if form == "raw":
        for k, n in enumerate(QUAT_NORMS):
            for side in range(4):  # child has the norm, parent has it, both have it, shared parent
                ri.append(row(("norm", n) if side != 1 else None))
                pi.append(row(("norm", n) if side != 0 else None) if side != 3 else pi[-1])
                w.append(TIE_WEIGHTS[(k + side) % len(TIE_WEIGHTS)])
                tie.append(n == 0)
                n_norm += 1
    Nq = len(quats)

    def edit(c, rng):
        for i, q in enumerate(quats):
            if q is None:
                continue
            if q[0] == "norm":
                d = rng.normal(size=4)
                q = (q[1] * d / np.linalg.norm(d)).astype(np.float64)
            c["rotation"][i] = np.asarray(q, F)
        c["fixed_quats"], c["norm_rows"] = fixed, n_norm

    return _case("ties", form, Nq + 4, 16, 2, ri, pi, w, 31, True, tie, edit)


# ---- the named cases -------------------------------------------------------------------------------

def _weights(form):
    lengths = [1, 2, 3, 5, 4] * 8
    c = _layout_case("weights", form, lengths, S=3, seed=41)
    c["w"] = np.asarray([WEIGHTS[k % len(WEIGHTS)] for k in range(len(c["ri"]))], F)
    return c


def _opacity_edges(form):
    lengths = [1, 2, 3] * 12
    c = _layout_case("opacity_edges", form, lengths, S=len(OPACITY_EDGES), seed=43)
    N = c["N"]
    rows = np.concatenate([c["ri"], np.unique(c["pi"]), np.arange(N - c["S"], N)])
    for k, r in enumerate(rows):  # children, parents and skybox rows all take every value
        c["opacity"][r, 0] = OPACITY_EDGES[k % len(OPACITY_EDGES)]
    return c


def _aaba(form):
    """A A B A, then the same across a wave edge and a 16-row edge, then A B A B."""
    rng = np.random.default_rng(47)
    lengths = [2, 1, 1] + [3] * 3 + [1] + [2, 1, 1] + [3] * 14 + [1, 1] + [2, 1, 1] + [1, 1, 1, 1]
    ri, pi, used = _sibling_layout(lengths, rng)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    for k in (0, 7, 26):      # runs k .. k + 2 are A A | B | A: the third takes the first's parent
        pi[starts[k + 2]:starts[k + 3]] = pi[starts[k]]
    k = len(lengths) - 4      # A B A B
    pi[starts[k + 2]] = pi[starts[k]]
    pi[starts[k + 3]] = pi[starts[k + 1]]
    return _case("aaba", form, used + 3 + 5, 16, 5, ri, pi, rng.uniform(0.05, 0.95, len(ri)), 47, True)


def _accumulating(name, form):
    """Layouts only the accumulating backward takes."""
    rng = np.random.default_rng(53)
    if name in ("roots_w025_S0", "roots_w025_S"):
        S = 0 if name.endswith("S0") else 4
        ri, pi, N = _sibling_layout([1, 1, 3, 1, 70, 1, 2], rng, roots=(0, 1, 3, 5))
        w = rng.uniform(0.05, 0.95, len(ri))
        w[pi < 0] = 0.25
        if S == 0:  # the row the roots read and write, N - 1, is a rendered row: swap it with row 0
            ri, pi = ((np.where(a == 0, N - 1, np.where(a == N - 1, 0, a))) for a in (ri, pi))
        return _case(name, form, N + S, 16, S, ri, pi, w, 53, False)
    R, N = 200, 260
    ri, pi = rng.permutation(N - 10)[:R], rng.integers(0, N - 10, R)
    if name == "child_is_parent":
        pi[::3] = ri[(np.arange(R)[::3] + 7) % R]
    elif name == "p_eq_c":
        pi[::4] = ri[::4]
    elif name == "child_twice":
        ri[100:] = ri[:100]
        ri[-1] = N - 1  # a rendered row that is also a skybox row
    return _case(name, form, N, 16, 6, ri, pi, rng.uniform(0.05, 0.95, R), 59, False)


ACCUMULATING = ("roots_w025_S0", "roots_w025_S", "child_is_parent", "p_eq_c", "child_twice")
NAMES = ("one_parent", "runs", "aaba", "split_by_skybox", "roots_w1", "ties", "weights",
         "opacity_edges") + ACCUMULATING


@functools.lru_cache(maxsize=None)
def case(name, form):
    assert form in FORMS
    if name == "one_parent":
        return _layout_case(name, form, [333], S=0, seed=3)
    if name == "runs":
        return _layout_case(name, form, _placed_runs(), S=7, seed=5)
    if name == "aaba":
        return _aaba(form)
    if name == "split_by_skybox":  # the last run ends at R = 200, inside a wave and a 16-row group
        return _layout_case(name, form, [5] * 35 + [25], S=41, seed=7)
    if name == "roots_w1":
        return _layout_case(name, form, [1, 1, 2, 1, 4, 1, 1, 60, 1], S=9, seed=9, roots=(0, 1, 3, 5, 6, 8))
    if name == "ties":
        return _ties(form)
    if name == "weights":
        return _weights(form)
    if name == "opacity_edges":
        return _opacity_edges(form)
    if name in ACCUMULATING:
        return _accumulating(name, form)
    raise KeyError(name)


def all_cases():
    return [case(n, f) for n in NAMES for f in FORMS]


def upstreams(c, seed=0, subset=(0, 1, 2, 3, 4)):
    """Finite float32 upstream gradients of the five outputs (None outside `subset`)."""
    rng = np.random.default_rng(seed + 17)
    rows = len(c["ri"]) + c["S"]
    shapes = ((rows, 3), (rows, 3), (rows, 4), (rows, 1), (rows, c["M"], 3))
    ups = [rng.normal(size=s).astype(F) for s in shapes]
    return [u if k in subset else None for k, u in enumerate(ups)]


# ---- hierarchies for the blend weight --------------------------------------------------------------

def _box(lo, hi, size):
    b = np.zeros((2, 4), F)
    b[0, :3], b[0, 3], b[1, :3] = lo, size, hi
    return b


def weight_hierarchy(n_children=2):
    """A root (node 0, the cube [-1, 1]^3, size 4) with n_children children whose boxes are the cube
    [-0.5, 0.5]^3 with sizes cycling through 4 (s = sp), 2 (s = sp / 2), 3 (in between) and 0.5.  Node k's
    Gaussian is k.  Seen from (d + 1, 0, 0) the root is at distance d and the children at d + 0.5."""
    n = 1 + n_children
    nodes = np.zeros((n, 7), np.int32)
    nodes[:, 2] = np.arange(n)
    nodes[:, 4] = 1
    nodes[0, 1], nodes[0, 5], nodes[0, 6] = -1, 1, n_children
    nodes[1:, 0], nodes[1:, 1], nodes[1:, 5] = 1, 0, -1
    boxes = np.zeros((n, 2, 4), F)
    boxes[0] = _box(-1, 1, 4)
    for k in range(1, n):
        boxes[k] = _box(-0.5, 0.5, (4, 2, 3, 0.5)[(k - 1) % 4])
    return nodes, boxes


def same_distance_hierarchy(n_children=4):
    """The children share the root's face x = 1, so both are at the same distance from a viewpoint on
    +x and s / sp is the ratio of the sizes: 1 (sp == s0, no blend), 1/2, 3/4, 1/8."""
    nodes, boxes = weight_hierarchy(n_children)
    for k in range(1, len(nodes)):
        boxes[k] = _box((0, -0.5, -0.5), (1, 0.5, 0.5), (4, 2, 3, 0.5)[(k - 1) % 4])
    return nodes, boxes


def weight_queries():
    """(name, nodes, boxes, viewpoint, target): the decisions of the rule on and next to their bounds.
    With the viewpoint at (1 + d, 0, 0), d a power of two, sp = 4 / d exactly."""
    up = lambda x: float(np.nextafter(F(x), F(np.inf)))
    dn = lambda x: float(np.nextafter(F(x), F(-np.inf)))
    H, Hs = weight_hierarchy(4), same_distance_hierarchy(4)
    q = []
    for d in (2.0, 4.0, 64.0):
        sp = 4.0 / d
        v = (1.0 + d, 0.0, 0.0)
        q += [(f"sp_eq_2target_d{d}", *Hs, v, sp / 2), (f"sp_above_2target_d{d}", *Hs, v, dn(sp / 2)),
              (f"sp_below_2target_d{d}", *Hs, v, up(sp / 2)),
              (f"target_eq_s0_d{d}", *Hs, v, sp * 0.75),
              (f"target_ge_sp_d{d}", *Hs, v, sp), (f"target_gt_sp_d{d}", *Hs, v, 2 * sp),
              (f"target_mid_d{d}", *Hs, v, sp * 0.625)]
    out_nodes, out_boxes = weight_hierarchy(2)  # children outside their parent: seen from inside the first,
    out_boxes[1] = _box((1.5, -0.5, -0.5), (2.5, 0.5, 0.5), 4)  # its s is FLT_MAX and sp is not; the second is at distance 1
    out_boxes[2] = _box((3, -0.5, -0.5), (4, 0.5, 0.5), 2)
    q += [("inside_parent", *H, (0.75, 0.0, 0.0), 8.0), ("inside_node_only", out_nodes, out_boxes, (2.0, 0.0, 0.0), 4.0),
          ("target_inf_inside_parent", *H, (0.75, 0.0, 0.0), float("inf")),
          ("on_parent_face", *H, (1.0, 0.0, 0.0), 8.0), ("on_parent_corner", *H, (1.0, -1.0, 1.0), 8.0),
          ("inside_node", *H, (0.25, 0.25, -0.25), 8.0), ("on_node_face", *H, (0.5, 0.0, 0.0), 8.0),
          ("just_outside_parent", *H, (up(1.0), 0.0, 0.0), 8.0),
          ("target_zero", *Hs, (5.0, 0.0, 0.0), 0.0), ("target_inf", *Hs, (5.0, 0.0, 0.0), float("inf")),
          ("target_inf_inside", *H, (0.25, 0.0, 0.0), float("inf"))]
    for n in (2, 254, 255, 256, 299):  # 3 to 300 nodes; every node queried, the root too
        q.append((f"nodes_{n + 1}", *same_distance_hierarchy(n), (5.0, 0.0, 0.0), 0.75))
    return q
