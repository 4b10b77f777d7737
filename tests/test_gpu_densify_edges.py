"""densify-and-prune on the device (csrc/densify.hip, gs_train/densify.py) at threshold ties,
overlapping predicates and edge sizes, and the statistics kernel (csrc/optim.hip) on NaN, Inf and
invisible rows, against the numpy float64 reference of tests/densify_ref.py on the inputs of
tests/densify_edge_cases.py (which tests/test_densify_cases_cpu.py shows to hold no row an fp32
evaluation may decide either way).

Exact: the counts, the shapes, the row map (the features hold 48 * source row + column), every
copied value, both Adam moments, the step entries, the zeroed statistics.  The split children's xyz
and scaling lie within densify_ref.child_bounds, derived there from the kernel's roundings; the
observed share of each bound goes to $GSR_PARITY_RECORD (profiles/r15_densify_edge_margins.jsonl)."""
from __future__ import annotations

import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import densify_edge_cases as EC  # noqa: E402
import densify_ref as DR  # noqa: E402
from helpers import record_margins  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATTR = {"xyz": "_xyz", "features": "_features", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}
GSR_OK, GSR_ERR_INVALID_ARGUMENT = 0, -1
CASES = EC.all_cases()


def _model(params, moments, accum, max_radii):
    from gs_train import Adam
    from gs_train.harness import GaussianSet
    P = params["xyz"].shape[0]
    g = GaussianSet(means3D=np.zeros((P, 3), np.float32), shs=np.zeros((P, 16, 3), np.float32),
                    opacities=np.full((P, 1), 0.5, np.float32), scales=np.ones((P, 3), np.float32),
                    rotations=np.zeros((P, 4), np.float32), device=DEV, joined_features=True)
    with torch.no_grad():
        for name, attr in ATTR.items():
            getattr(g, attr).copy_(torch.tensor(np.asarray(params[name], np.float32), device=DEV))
    _set_stats(g, accum, max_radii)
    opt = Adam(g.param_groups(), lr=0.0, eps=1e-15)
    for name, (m, v) in moments.items():
        opt.state[getattr(g, ATTR[name])] = {"step": torch.tensor(7.0), "exp_avg": torch.tensor(m, device=DEV),
                                             "exp_avg_sq": torch.tensor(v, device=DEV)}
    return g, opt


def _set_stats(g, accum, max_radii):
    g.xyz_gradient_accum = torch.tensor(np.asarray(accum, np.float32).reshape(-1, 1), device=DEV)
    g.max_radii2D = torch.tensor(np.asarray(max_radii, np.float32).reshape(-1), device=DEV)
    g.denom = torch.full((g.P, 1), 3.0, device=DEV)


def _densify(g, opt, case, normals):
    from gs_train.densify import densify_and_prune
    from gs_train.gtcloud import GtPointCloud
    s = case["scalars"]
    cloud = GtPointCloud(case["cloud"], threshold=case["thr"], device=DEV) if "cloud" in case else None
    try:
        return densify_and_prune(g, opt, s["max_grad"], s["min_opacity"], s["extent"], s["percent_dense"],
                                 first_row=s["first_row"], normals=torch.tensor(normals, device=DEV), gt_cloud=cloud)
    finally:
        if cloud is not None:
            cloud.close()


def _np(t):
    return t.detach().cpu().numpy()


def _compare(name, g, opt, c, ref, with_moments):
    """Everything the module's docstring lists, against one densify_ref result; returns the largest
    shares of the children's bounds."""
    want = dict(ref["counts"])
    for k in ("gt_pruned", "gt_pruned_fixed"):
        if k in ref:
            want[k] = ref[k]
    assert c == want, (name, c, want)
    total = want["total"]
    assert g.P == total
    got = {n: _np(getattr(g, a)) for n, a in ATTR.items()}
    for n in DR.PARAMS:
        assert got[n].shape == (total,) + tuple(np.asarray(ref["params"][n]).shape[1:]), (name, n, got[n].shape)
    # the row map, through the features
    f = got["features"].reshape(total, 48)
    rf = ref["params"]["features"].reshape(total, 48).astype(np.float32)
    np.testing.assert_array_equal(f[:, 0].astype(np.int64) // 48, rf[:, 0].astype(np.int64) // 48,
                                  err_msg=f"{name}: row map")
    np.testing.assert_array_equal(f, rf, err_msg=name)
    for n in ("opacity", "rotation"):
        np.testing.assert_array_equal(got[n], ref["params"][n].astype(np.float32), err_msg=f"{name}: {n}")
    child = ref["child"]
    share = {}
    for n, bound in (("xyz", ref["child_bound_xyz"]), ("scaling", ref["child_bound_scaling"])):
        r64 = ref["params"][n]
        np.testing.assert_array_equal(got[n][~child], r64[~child].astype(np.float32), err_msg=f"{name}: {n} copies")
        gc, rc = got[n][child].astype(np.float64), r64[child]
        nan = np.isnan(rc)
        np.testing.assert_array_equal(np.isnan(gc), nan, err_msg=f"{name}: {n} NaN rows")  # a zero quaternion
        with np.errstate(invalid="ignore"):
            e = np.where(nan, 0.0, np.abs(gc - rc) / bound)
        share[n] = float(e.max()) if e.size else 0.0
    for n, attr in ATTR.items():
        p = getattr(g, attr)
        assert isinstance(p, torch.nn.Parameter)
        assert sum(q is p for grp in opt.param_groups for q in grp["params"]) == 1, (name, n, "group")
        if n in with_moments:
            st = opt.state[p]
            for k, key in enumerate(("exp_avg", "exp_avg_sq")):
                assert st[key].shape == p.shape
                np.testing.assert_array_equal(_np(st[key]), ref["moments"][n][k].astype(np.float32).reshape(p.shape),
                                              err_msg=f"{name}: {n} {key}")
            assert float(st["step"]) == 7.0
        else:
            assert p not in opt.state, (name, n)
    assert len(opt.state) == len(with_moments)
    for t, shape in ((g.xyz_gradient_accum, (total, 1)), (g.denom, (total, 1)), (g.max_radii2D, (total,))):
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and not bool(t.any())
    record_margins(f"densify_edges/{name}", xyz_share=share["xyz"], scaling_share=share["scaling"],
                   children=float(child.sum()))
    print(f"{name}: children {int(child.sum())} xyz share {share['xyz']:.3f} scaling share {share['scaling']:.3f}")
    assert share["xyz"] <= 1.0 and share["scaling"] <= 1.0, (name, share)
    return share


@pytest.mark.parametrize("name", list(CASES))
def test_densify_edge_case_matches_float64_reference(name):
    case = CASES[name]()
    ref, normals = EC.reference(case)
    g, opt = _model(case["params"], case["moments"], case["accum"], case["max_radii"])
    before = {n: _np(getattr(g, a)).copy() for n, a in ATTR.items()}
    for n in DR.PARAMS:  # the model holds the case's numbers bit for bit
        np.testing.assert_array_equal(before[n], case["params"][n])
    c = _densify(g, opt, case, normals)
    _compare(name, g, opt, c, ref, set(case["moments"]))
    if name == "extremes_nothing":  # every array and moment is bit-identical to its input
        for n, a in ATTR.items():
            assert _np(getattr(g, a)).tobytes() == before[n].tobytes()
            for k, key in enumerate(("exp_avg", "exp_avg_sq")):
                assert _np(opt.state[getattr(g, a)][key]).tobytes() == case["moments"][n][k].tobytes()
    if name in ("extremes_all_pruned", "extremes_empty"):
        assert c["total"] == 0 and c["split"] == 0 and g._features.shape == (0, 16, 3)
        assert opt.state[g._xyz]["exp_avg"].shape == (0, 3)
    if name == "quaternions":
        x = _np(g._xyz)
        assert np.isnan(x[[EC.QUAT_ZERO_ROW, 64 + EC.QUAT_ZERO_ROW]]).all() and np.isnan(x).any(axis=1).sum() == 2


def test_two_events_in_a_row_match_the_reference_applied_twice():
    case = EC.sizes(257)
    ref, normals = EC.reference(case)
    g, opt = _model(case["params"], case["moments"], case["accum"], case["max_radii"])
    c = _densify(g, opt, case, normals)
    _compare("twice/first", g, opt, c, ref, set(case["moments"]))
    # the second event starts from what the device holds (the children an ulp or two from float64's)
    p2 = {n: _np(getattr(g, a)).copy() for n, a in ATTR.items()}
    m2 = {n: tuple(_np(opt.state[getattr(g, a)][k]).copy() for k in ("exp_avg", "exp_avg_sq")) for n, a in ATTR.items()}
    accum, maxr = EC.second_stats(p2, seed=5)
    _set_stats(g, accum, maxr)
    args = EC.run_args(case)
    n2 = DR.plan(p2, accum, maxr, **args)["counts"]["split"]
    z2 = EC.normals_for(n2, seed=1)
    ref2 = DR.densify_ref(p2, m2, accum, maxr, z2, **args)
    assert ref2["counts"]["cloned"] > 0 and ref2["counts"]["split"] > 0 and ref2["counts"]["kept"] < p2["xyz"].shape[0]
    # the features still name the first event's sources, a clone and its source alike: the second
    # map is checked through them and, for such twins, through the moments (zero on the clone)
    c2 = _densify(g, opt, case, z2)
    _compare("twice/second", g, opt, c2, ref2, set(case["moments"]))


# ---- the C ABI's edges ---------------------------------------------------------------------------

def _abi_groups(P0, total, widths=(3, 48, 1, 3, 4), dst_widths=None):
    from diff_gaussian_rasterization._lib import RowGroup
    src = (RowGroup * len(widths))()
    dst = (RowGroup * len(widths))()
    keep = []
    for k, w in enumerate(widths):
        a = torch.zeros((max(P0, 1), w), device=DEV)
        b = torch.full((max(total, 1), w), -7.0, device=DEV)
        keep += [a, b]
        src[k] = RowGroup(a.data_ptr(), None, None, w)
        dst[k] = RowGroup(b.data_ptr(), None, None, (dst_widths or widths)[k])
    return src, dst, keep


def test_c_abi_rejects_bad_arguments_and_launches_nothing_for_no_rows():
    from gs_train._native import lib, ptr, stream
    L = lib()
    P0 = 8
    scratch = torch.zeros(max(1, L.gsr_densify_scratch_bytes(P0)), dtype=torch.uint8, device=DEV)
    s = stream(scratch.device)
    counts = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    col = torch.zeros(P0, device=DEV)
    s3 = torch.zeros((P0, 3), device=DEV)
    plan = lambda first: L.gsr_densify_plan(P0, first, ptr(col), ptr(col), ptr(col), ptr(s3), 0.5, 0.5, 1.0,
                                            ptr(scratch), ptr(counts), s)
    assert plan(-1) == GSR_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert counts.tolist() == [-1] * 4  # nothing ran
    assert plan(0) == GSR_OK and plan(P0 + 5) == GSR_OK
    torch.cuda.synchronize()
    assert counts.tolist() == [P0, 0, 0, P0]  # zero rows: kept, nothing selected (g = 0)

    def apply(total, **kw):
        src, dst, keep = _abi_groups(P0, total, **kw)
        rc = L.gsr_densify_apply(P0, 5, src, dst, 0, 3, 4, ctypes.c_void_p(0), 0, ptr(scratch), total, s)
        torch.cuda.synchronize()
        return rc, keep
    assert apply(3 * P0 + 1)[0] == GSR_ERR_INVALID_ARGUMENT                                   # more rows than a plan makes
    assert apply(P0, dst_widths=(3, 47, 1, 3, 4))[0] == GSR_ERR_INVALID_ARGUMENT               # a width mismatch
    assert apply(P0, widths=(3, 48, 1, 4, 4))[0] == GSR_ERR_INVALID_ARGUMENT                   # scaling is 3 wide
    rc, keep = apply(0)
    assert rc == GSR_OK and all(bool((b == -7.0).all()) for b in keep[1::2])                   # nothing written
    rc, keep = apply(P0)  # the plan above kept every row: a plain copy, and the last check of the layout
    assert rc == GSR_OK and all(bool((b == 0.0).all()) for b in keep[1::2])


# ---- the statistics ------------------------------------------------------------------------------

@pytest.mark.parametrize("P", EC.STATS_SIZES)
def test_densify_stats_on_nan_inf_and_invisible_rows(P):
    from gs_train import add_densification_stats
    d = EC.stats_inputs(P)
    t = lambda k: torch.tensor(d[k], device=DEV).contiguous()
    mr, acc, den = t("max_r"), t("accum"), t("denom")
    add_densification_stats(t("radii"), t("grad2d"), mr, acc, den)
    rm, ra, rd = DR.stats_ref(d["radii"], d["grad2d"], d["max_r"], d["accum"], d["denom"])
    mr, acc, den = _np(mr), _np(acc), _np(den)
    hidden = d["radii"] <= 0
    for got, was in ((mr, d["max_r"]), (acc, d["accum"]), (den, d["denom"])):  # radius 0 or negative: untouched
        assert got[hidden].tobytes() == was[hidden].tobytes()
    np.testing.assert_array_equal(mr, rm.astype(np.float32))
    np.testing.assert_array_equal(den, rd.astype(np.float32))
    np.testing.assert_array_equal(np.isnan(acc), np.isnan(ra), err_msg="NaN placement (torch.max propagates NaN)")
    np.testing.assert_array_equal(np.isinf(acc), np.isinf(ra))
    fin = np.isfinite(ra)
    np.testing.assert_allclose(acc[fin], ra[fin], rtol=2e-7, atol=0)
    tie = d["kinds"] == 2  # n == accum == 5 exactly
    assert (acc[tie] == 5.0).all()
