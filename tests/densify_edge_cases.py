"""Seeded inputs for densify-and-prune at threshold ties, overlapping predicates and edge sizes
(csrc/densify.hip, gs_train/densify.py).  tests/test_gpu_densify_edges.py runs the kernels on these
against tests/densify_ref.py; tests/test_densify_cases_cpu.py checks that every case has no
undecided row, that the populations it names exist and that the tie rows get the outcome the
reference source's operators give.  Importable without a GPU and without torch.

A case is a dict: params (PARAMS of densify_ref, float32; features (P, 16, 3) holding 48 * row +
column, so that an output row names its source), moments ({name: (exp_avg, exp_avg_sq)} for the
parameters with Adam state, or "none" for an optimizer with no state at all), accum (P, 1),
max_radii (P,), scalars (max_grad, min_opacity, extent, percent_dense, first_row), ties ({row:
(clone, split, prune)}: the constructed exact ties and their one-step neighbours with the outcome
the source's >=, >, <=, < give), and for the cloud case cloud and thr.

Exact ties are exact in fp32 under any implementation whose expf, divide and powf are exact on
exactly representable results:
    s_raw = 0    exp = 1, so smax == max_scale == 1 (percent_dense 0.5, extent 2): a clone, no split
    o_raw = 0    op = 1 / (1 + 1) = 0.5 == min_opacity: not pruned
    o_raw = 40   exp(-40) = 4e-18 vanishes beside 1 in fp32 and in float64 (at 20 it does in fp32
                 only, and the float64 reference would see op = 1 - 2e-9): op = 1, op^0.2 = 1; with
                 g = 0.25, r = 2 the product is exactly 0.5 == max_grad: selected; g one float32
                 below 0.25 gives the float32 below 0.5: not selected
The 0.15 eligibility threshold cannot be met exactly through a sigmoid: rows sit at
op = 0.15 (1 +- 2^-12), far outside UNDECIDED_REL."""
from __future__ import annotations

import numpy as np

import densify_ref as DR

DEFAULT = dict(max_grad=0.0002, min_opacity=0.05, extent=200.0, percent_dense=0.0001, first_row=0)
TIE = dict(max_grad=0.5, min_opacity=0.5, extent=2.0, percent_dense=0.5, first_row=0)  # max_scale 1
SIZES = (1, 2, 255, 256, 257, 1025, 4099)
SCAFFOLD_P = 700
SCAFFOLD_FIRST = (0, 1, SCAFFOLD_P // 2, SCAFFOLD_P, SCAFFOLD_P + 5)
EXTREMES = ("nothing", "all_pruned", "all_split", "all_cloned", "empty")
NO_STATE = ("none", "some")
STATS_SIZES = (1, 255, 257)


def _logit(p):
    return float(np.log(p / (1.0 - p)))


def _population(rng, P, scalars, o_sd=2.0):
    """Ordinary rows around the case's thresholds: about a fifth not eligible, both sizes, gradient
    quantities on both sides of max_grad."""
    t = DR.thresholds(scalars["max_grad"], scalars["min_opacity"], scalars["extent"], scalars["percent_dense"])
    ls = np.log(t["max_scale"])
    r_max = 20.0
    g_max = 8.0 * t["max_grad"] / r_max
    return dict(opacity=rng.normal(0.0, o_sd, (P, 1)).astype(np.float32),
                scaling=rng.normal(ls - 0.6, 0.7, (P, 3)).astype(np.float32),
                accum=rng.uniform(0.0, g_max, (P, 1)).astype(np.float32),
                max_radii=rng.uniform(0.0, r_max, P).astype(np.float32))


def _finish(name, rng, pop, scalars, ties=None, moments="all", fixed=(), **extra):
    """Adds xyz, rotation, the row-naming features and the moments; redraws every undecided row
    that is neither a tie nor otherwise constructed (`fixed`) until none is left."""
    P = pop["opacity"].shape[0]
    ties = dict(ties or {})
    args = (scalars["max_grad"], scalars["min_opacity"], scalars["extent"], scalars["percent_dense"],
            scalars["first_row"])
    for _ in range(50):
        bad = DR.undecided(pop["opacity"], pop["scaling"], pop["accum"], pop["max_radii"], *args, exact_ties=ties)
        if bad.size == 0:
            break
        assert not set(bad.tolist()) & set(fixed), (name, "a constructed row is undecided", bad)
        new = _population(rng, bad.size, scalars)
        for k in new:
            pop[k][bad] = new[k]
    else:
        raise AssertionError(f"{name}: undecided rows remain")
    params = dict(xyz=pop.get("xyz", (rng.normal(size=(P, 3)) * 5).astype(np.float32)),
                  features=(48.0 * np.arange(P)[:, None] + np.arange(48)[None]).astype(np.float32).reshape(P, 16, 3),
                  opacity=pop["opacity"], scaling=pop["scaling"],
                  rotation=pop.get("rotation", rng.normal(size=(P, 4)).astype(np.float32)))
    names = DR.PARAMS if moments == "all" else ("xyz", "opacity") if moments == "some" else ()
    mom = {n: (rng.normal(size=params[n].shape).astype(np.float32),
               rng.uniform(0.0, 1.0, params[n].shape).astype(np.float32)) for n in names}
    return dict(name=name, params=params, moments=mom, no_state=moments == "none", accum=pop["accum"],
                max_radii=pop["max_radii"], scalars=dict(scalars), ties=ties, **extra)


def run_args(case):
    """The positional arguments of densify_ref.plan / densify_ref after `params`, bar the normals."""
    s = case["scalars"]
    return dict(max_grad=s["max_grad"], min_opacity=s["min_opacity"], extent=s["extent"],
                percent_dense=s["percent_dense"], first_row=s["first_row"], cloud=case.get("cloud"),
                thr=case.get("thr"))


def normals_for(n_split, seed=0):
    """(2 n_split, 3) standard-normal draws, every row distinct: a wrong rank moves a child by about
    exp(s), eight orders above its bound."""
    return np.random.default_rng(9000 + seed).normal(size=(2 * int(n_split), 3)).astype(np.float32)


def reference(case, normals=None):
    """densify_ref on the case, with normals_for(n_split) unless given."""
    a = run_args(case)
    if normals is None:
        n = DR.plan(case["params"], case["accum"], case["max_radii"], **a)["counts"]["split"]
        normals = normals_for(n)
    return DR.densify_ref(case["params"], case["moments"], case["accum"], case["max_radii"], normals, **a), normals


# ---- the cases -----------------------------------------------------------------------------------

def sizes(P):
    rng = np.random.default_rng(100 + P)
    return _finish(f"sizes_{P}", rng, _population(rng, P, DEFAULT), DEFAULT)


def _put(pop, i, o, s, g, r):
    pop["opacity"][i, 0], pop["scaling"][i], pop["accum"][i, 0], pop["max_radii"][i] = o, s, g, r


def ties(min_opacity=0.5):
    """P0 = 300 under the TIE scalars (max_grad 0.5, max_scale 1, min_opacity 0.5, or 0.05 for
    ties_low, where the rows either side of op = 0.15 are not pruned and so show as clone / kept)."""
    sc = dict(TIE, min_opacity=min_opacity)
    rng = np.random.default_rng(41 if min_opacity == 0.5 else 42)
    P = 300
    pop = _population(rng, P, sc)
    below = np.nextafter(np.float32(0.25), np.float32(0))
    small, tie_s, big = (-1.0, -2.0, -0.5), (-1.0, 0.0, -2.0), (-1.0, 0.01, -2.0)
    lo, hi = _logit(0.15 * (1 - 2.0 ** -12)), _logit(0.15 * (1 + 2.0 ** -12))
    pr_lo = 0.15 < min_opacity       # the rows around op = 0.15 are below min_opacity in the 0.5 case
    rows = [
        # (o, s, g, r) -> (clone, split, prune)
        ((40.0, tie_s, 1.0, 2.0), (True, False, False)),       # smax == max_scale: <= holds, > does not
        ((40.0, big, 1.0, 2.0), (False, True, False)),         # clearly above: split
        ((0.0, small, 0.0, 2.0), (False, False, False)),  # op == min_opacity 0.5: < does not hold
        ((0.0, small, 1.0, 2.0), (True, False, False)),   # the same, selected: the clone is kept too
        ((0.0, big, 1.0, 2.0), (False, True, False)),     # and as a split row: both children kept
        ((-1e-3, small, 1.0, 2.0), (True, False, min_opacity == 0.5)),  # op = 0.49975: pruned with its clone
        ((40.0, small, 0.25, 2.0), (True, False, False)),      # c == max_grad: >= holds (clone)
        ((40.0, big, 0.25, 2.0), (False, True, False)),        # c == max_grad: >= holds (split)
        ((40.0, small, below, 2.0), (False, False, False)),    # one float32 below: not selected
        ((40.0, big, below, 2.0), (False, False, False)),
        ((40.0, tie_s, 0.25, 2.0), (True, False, False)),      # both ties at once
        ((0.0, tie_s, 0.25 * 2.0, 2.0), (True, False, False)),  # op and scale ties, c = 0.87 > 0.5
        ((hi, small, 2.0, 2.0), (True, False, pr_lo)),         # op just above 0.15: eligible
        ((hi, big, 2.0, 2.0), (False, True, pr_lo)),
        ((lo, small, 2.0, 2.0), (False, False, pr_lo)),        # op just below 0.15: not eligible
        ((lo, big, 2.0, 2.0), (False, False, pr_lo)),
    ]
    tie_rows = {}
    # twice each: once inside the first block, once across the second (rows 250 ..)
    for rep, base in enumerate((7, 250)):
        for k, ((o, s, g, r), want) in enumerate(rows):
            i = base + 3 * k
            _put(pop, i, o, s, g, r)
            tie_rows[i] = want
    name = "ties" if min_opacity == 0.5 else "ties_low"
    return _finish(name, rng, pop, sc, ties=tie_rows)


def overlap():
    """min_opacity 0.6: rows with 0.15 < op < 0.6 are selected and pruned at once, so kept split rows
    (Cnt4::k) are fewer than split rows (Cnt4::s), interleaved with them, and clones are dropped."""
    sc = dict(DEFAULT, min_opacity=0.6)
    rng = np.random.default_rng(51)
    return _finish("overlap", rng, _population(rng, 1000, sc, o_sd=1.5), sc)


def scaffold(first_row):
    """One P0 = 700 population; its first rows are forced through clone, split and prune candidates in
    turn, so every first_row > 0 shields some of each."""
    sc = dict(DEFAULT, first_row=first_row)
    rng = np.random.default_rng(61)
    pop = _population(rng, SCAFFOLD_P, sc)
    ls = float(np.log(DR.thresholds(**{k: sc[k] for k in ("max_grad", "min_opacity", "extent", "percent_dense")})
                      ["max_scale"]))
    fixed = []
    for i in range(0, SCAFFOLD_P, 7):  # every seventh row, the whole length: below any first_row > 0
        kind = (i // 7) % 3
        if kind == 0:
            _put(pop, i, 2.0, (ls - 1, ls - 2, ls - 1), 1e-3, 10.0)   # would clone
        elif kind == 1:
            _put(pop, i, 2.0, (ls + 1, ls - 2, ls - 1), 1e-3, 10.0)   # would split
        else:
            _put(pop, i, -5.0, (ls - 1, ls - 2, ls - 1), 0.0, 10.0)   # would be pruned
        fixed.append(i)
    return _finish(f"scaffold_{first_row}", rng, pop, sc, fixed=fixed)


def extremes(which):
    sc = dict(DEFAULT)
    rng = np.random.default_rng(71)
    P = 0 if which == "empty" else 300
    pop = _population(rng, P, sc)
    ls = float(np.log(DR.thresholds(sc["max_grad"], sc["min_opacity"], sc["extent"], sc["percent_dense"])["max_scale"]))
    if which == "nothing":
        pop["accum"][:] = 0.0
        pop["opacity"][:] = np.abs(pop["opacity"])  # op >= 0.5: nothing pruned
    elif which == "all_pruned":
        pop["opacity"][:] = -6.0 - np.abs(pop["opacity"])  # op < 0.0025
    elif which in ("all_split", "all_cloned"):
        pop["opacity"][:] = 1.0 + np.abs(pop["opacity"])
        pop["accum"][:] = 1e-3 + pop["accum"]
        pop["max_radii"][:] = 5.0 + pop["max_radii"]
        dev = np.abs(pop["scaling"] - (ls - 0.6))
        pop["scaling"][:] = ls + 0.5 + dev if which == "all_split" else ls - 0.5 - dev
    return _finish(f"extremes_{which}", rng, pop, sc, fixed=range(P))


ACC_ROWS = {  # row -> (g, r, small scale?) in the accumulator case; all op = sigmoid(2)
    10: (np.nan, 10.0, True), 11: (np.nan, 10.0, False),        # NaN -> 0: kept
    20: (np.inf, 0.0, True), 21: (np.inf, 0.0, False),          # Inf * 0 = NaN: compares false, kept
    30: (np.inf, 3.0, True), 31: (np.inf, 3.0, False),          # Inf >= max_grad: clone / split
    40: (0.0, 10.0, True), 41: (0.0, 10.0, False),              # kept
    50: (1e-40, 10.0, True), 51: (1e-40, 10.0, False),          # denormal: kept
    60: (-1.0, 10.0, True), 61: (-1.0, 10.0, False),            # negative: |g| clones, g never splits
    62: (-1e-3, 10.0, True), 63: (-1e-3, 10.0, False),
    70: (1.0, 0.0, True), 71: (1.0, 0.0, False),                # max_radii2D = 0: kept
    260: (np.nan, 10.0, False), 261: (-1.0, 10.0, True), 262: (-1.0, 10.0, False), 263: (np.inf, 3.0, False),
}


def accumulator():
    sc = dict(DEFAULT)
    rng = np.random.default_rng(81)
    pop = _population(rng, 300, sc)
    ls = float(np.log(DR.thresholds(sc["max_grad"], sc["min_opacity"], sc["extent"], sc["percent_dense"])["max_scale"]))
    for i, (g, r, small) in ACC_ROWS.items():
        _put(pop, i, 2.0, (ls - 1, ls - 2, ls - 1) if small else (ls - 1, ls + 1, ls - 2), g, r)
    return _finish("accumulator", rng, pop, sc, fixed=list(ACC_ROWS))


def accumulator_expected():
    """row -> (clone, split, prune) by the source's expressions."""
    out = {}
    for i, (g, r, small) in ACC_ROWS.items():
        sel_abs = (np.isinf(g) and r > 0) or (np.isfinite(g) and abs(g) * r > 1e-3)
        sel = sel_abs and g > 0
        out[i] = (bool(sel_abs and small), bool(sel and not small), False)
    return out


def zero_threshold():
    """max_grad = 0: a NaN accumulator is zeroed first (grads[grads.isnan()] = 0) and 0 >= 0 selects
    the row, where a NaN left in place would compare false.  0 * r * op^0.2 is exactly 0 in any
    arithmetic, so the rows with g = NaN or g = 0 are exact ties; the others have g > 0."""
    sc = dict(DEFAULT, max_grad=0.0)
    rng = np.random.default_rng(85)
    P = 70
    pop = _population(rng, P, DEFAULT)
    pop["accum"] = rng.uniform(1e-5, 1e-4, (P, 1)).astype(np.float32)
    pop["max_radii"] = rng.uniform(1.0, 20.0, P).astype(np.float32)
    pop["accum"][0::5] = np.nan
    pop["accum"][1::5] = 0.0
    exact = [i for i in range(P) if i % 5 < 2]
    case = _finish("zero_threshold", rng, pop, sc, ties={i: None for i in exact}, fixed=range(P))
    op, _, _, smax = DR.quantities(pop["opacity"], pop["scaling"], pop["accum"], pop["max_radii"])
    ms = DR.thresholds(0.0, sc["min_opacity"], sc["extent"], sc["percent_dense"])["max_scale"]
    for i in exact:  # selected whenever eligible: the operator is >=
        el = op[i] > DR.OP_ELIGIBLE
        case["ties"][i] = (bool(el and smax[i] <= ms), bool(el and smax[i] > ms), bool(op[i] < 0.05))
    return case


QUAT_ZERO_ROW = 5


def quaternions():
    """64 rows, every one split (max_scale 1e-6): |q| from 1e-3 to 1e3, row 5 a zero quaternion (NaN
    children, here and in the reference), s_raw over [-12, 4], |xyz| up to 1e4."""
    sc = dict(DEFAULT, extent=0.01)  # max_scale = 1e-6, ln = -13.8
    rng = np.random.default_rng(91)
    P = 64
    pop = _population(rng, P, sc)
    pop["opacity"][:] = 2.0
    pop["accum"][:] = 1.0
    pop["max_radii"][:] = 5.0
    pop["scaling"] = rng.uniform(-12.0, 4.0, (P, 3)).astype(np.float32)
    q = rng.normal(size=(P, 4))
    q *= (10.0 ** np.linspace(-3.0, 3.0, P) / np.linalg.norm(q, axis=1))[:, None]
    q[QUAT_ZERO_ROW] = 0.0
    q[6] = (1e3, 0.0, 0.0, 0.0)  # the identity, far from unit length
    q[7] = (0.0, 0.0, 1e-3, 0.0)  # a half turn about y
    pop["rotation"] = q.astype(np.float32)
    pop["xyz"] = (rng.uniform(-1.0, 1.0, (P, 3)) * 10.0 ** rng.uniform(0.0, 4.0, (P, 1))).astype(np.float32)
    return _finish("quaternions", rng, pop, sc, fixed=range(P))


def no_state(which):
    rng = np.random.default_rng(111)
    return _finish(f"no_state_{which}", rng, _population(rng, 257, DEFAULT), DEFAULT, moments=which)


def cloud():
    """P0 = 600, first_row 100, a 200-point cloud in [0, 4]^2 x [0, 1] with thr 0.3.  A third of the rows
    sit within 0.09 of a cloud point (d2 <= 0.0075 against thr^2 = 0.09), a third 5 above the slab
    inside the bounds (d2 >= 16), a third outside the XY bounds; independent of the predicates."""
    sc = dict(DEFAULT, first_row=100)
    rng = np.random.default_rng(121)
    P = 600
    pop = _population(rng, P, sc)
    pts = rng.uniform((0.0, 0.0, 0.0), (4.0, 4.0, 1.0), (200, 3)).astype(np.float32)
    where = rng.integers(0, 3, P)
    xyz = np.empty((P, 3))
    near = pts[rng.integers(0, 200, P)].astype(np.float64) + rng.uniform(-0.05, 0.05, (P, 3))
    far = np.concatenate([rng.uniform(1.0, 3.0, (P, 2)), rng.uniform(5.0, 6.0, (P, 1)) + 1.0], axis=1)
    outside = far + np.array([10.0, 0.0, 0.0])
    for k, src in enumerate((near, far, outside)):
        xyz[where == k] = src[where == k]
    pop["xyz"] = xyz.astype(np.float32)
    return _finish("cloud", rng, pop, sc, cloud=pts, thr=0.3, where=where)


def second_stats(params, seed, scalars=DEFAULT):
    """Fresh statistics (accum (P, 1), max_radii (P,)) for a second event on `params` (float32, the
    first event's output), with no undecided row: the statistics are redrawn, the parameters stay."""
    rng = np.random.default_rng(seed)
    P = params["opacity"].shape[0]
    pop = _population(rng, P, scalars)
    accum, maxr = pop["accum"], pop["max_radii"]
    args = (scalars["max_grad"], scalars["min_opacity"], scalars["extent"], scalars["percent_dense"],
            scalars["first_row"])
    for _ in range(50):
        bad = DR.undecided(params["opacity"], params["scaling"], accum, maxr, *args)
        if bad.size == 0:
            return accum, maxr
        new = _population(rng, bad.size, scalars)
        accum[bad], maxr[bad] = new["accum"], new["max_radii"]
    # only the statistics can be redrawn: an op or smax on a threshold stays
    raise AssertionError("second_stats: a parameter of the first event's output is undecided")


def all_cases():
    """Every case by name (built on demand)."""
    out = {f"sizes_{P}": (lambda P=P: sizes(P)) for P in SIZES}
    out["ties"] = ties
    out["ties_low"] = lambda: ties(0.05)
    out["overlap"] = overlap
    out.update({f"scaffold_{f}": (lambda f=f: scaffold(f)) for f in SCAFFOLD_FIRST})
    out.update({f"extremes_{w}": (lambda w=w: extremes(w)) for w in EXTREMES})
    out["accumulator"] = accumulator
    out["zero_threshold"] = zero_threshold
    out["quaternions"] = quaternions
    out.update({f"no_state_{w}": (lambda w=w: no_state(w)) for w in NO_STATE})
    out["cloud"] = cloud
    return out


# ---- the larger random state of tests/test_gpu_densify.py ----------------------------------------
STATE_ARGS = (0.005, 0.05, 200.0, 0.0001, 300)  # max_grad, min_opacity, extent, percent_dense, first_row


def state_arrays(P, seed):
    """The draws of test_gpu_densify._state, in its order, and the generator for what follows them;
    opacity_raw / scaling_raw are GaussianSet's inverse activations in numpy float32 (the model's own
    are torch's, an ulp apart at most: immaterial to a count of undecided rows)."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(P, 4)).astype(np.float32)
    a = dict(means3D=rng.normal(size=(P, 3)).astype(np.float32) * 5,
             shs=rng.normal(size=(P, 16, 3)).astype(np.float32),
             opacities=rng.uniform(0.01, 0.99, (P, 1)).astype(np.float32),
             scales=np.exp(rng.normal(-4.0, 0.5, (P, 3))).astype(np.float32), rotations=q)
    acc = rng.uniform(0, 0.001, (P, 1)).astype(np.float32)
    acc[::97] = np.nan  # NaN accumulators are zeroed first
    a.update(accum=acc, max_radii=rng.uniform(0, 20, P).astype(np.float32))
    op = np.clip(a["opacities"], np.float32(1e-6), np.float32(1 - 1e-6))
    a.update(opacity_raw=np.log(op / (1 - op)), scaling_raw=np.log(a["scales"]))
    return a, rng


# ---- the statistics kernel -----------------------------------------------------------------------

def stats_inputs(P):
    """radii (int32), grad2d (P, 3), max_r, accum, denom with, cyclically by row: an invisible row
    (radius 0, then negative), n == accum exactly (3-4-5), gx NaN, gy NaN, accum NaN with a finite
    gradient, +Inf gx, accum above n, accum below n."""
    rng = np.random.default_rng(200 + P)
    radii = rng.integers(1, 40, P).astype(np.int32)
    g = (rng.normal(size=(P, 3)) * 1e-3).astype(np.float32)
    max_r = rng.uniform(0.0, 40.0, P).astype(np.float32)
    accum = rng.uniform(0.0, 2e-3, P).astype(np.float32)
    denom = rng.integers(0, 5, P).astype(np.float32)
    kinds = np.arange(P) % 9 if P > 1 else np.array([4])
    for i, k in enumerate(kinds):
        if k == 0:
            radii[i] = 0
        elif k == 1:
            radii[i] = -3
        elif k == 2:
            g[i, :2], accum[i] = (3.0, 4.0), 5.0
        elif k == 3:
            g[i, 0] = np.nan
        elif k == 4:
            g[i, 1] = np.nan
        elif k == 5:
            accum[i] = np.nan
        elif k == 6:
            g[i, 0] = np.inf
    return dict(radii=radii, grad2d=g, max_r=max_r, accum=accum, denom=denom, kinds=kinds)
