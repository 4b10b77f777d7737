"""The float64 reference of densify-and-prune (tests/densify_ref.py) and the edge cases
(tests/densify_edge_cases.py), checked without a GPU:

* densify_ref reproduces the four committed runs of the reference's own densify_and_prune
  (tests/golden/densify_prune_*.npz, with and without the ground-truth cloud): counts and row order
  exactly, copied rows and moments bit for bit after the float32 cast, the split children within
  densify_ref.child_bounds -- which ties the reference to the real program, not to our kernel;
* every case has zero undecided rows, every population it names exists, and the tie rows get the
  outcome the reference source's comparison operators give."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import densify_edge_cases as EC  # noqa: E402
import densify_ref as DR  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = EC.all_cases()


def _fixture(case, gt):
    d = dict(np.load(os.path.join(GOLD, f"densify_prune_{case}.npz")))
    if gt:
        d.update(np.load(os.path.join(GOLD, f"densify_prune_gt_{case}.npz")))
    params = dict(xyz=d["in_xyz"], features=np.concatenate((d["in_f_dc"], d["in_f_rest"]), 1),
                  opacity=d["in_opacity"], scaling=d["in_scaling"], rotation=d["in_rotation"])
    keys = {"xyz": ("xyz",), "features": ("f_dc", "f_rest"), "opacity": ("opacity",), "scaling": ("scaling",),
            "rotation": ("rotation",)}
    cat = lambda pre, ks: np.concatenate([d[pre + k] for k in ks], 1)
    moments = {n: (cat("in_m_", ks), cat("in_v_", ks)) for n, ks in keys.items()}
    want = {n: cat("out_", ks) for n, ks in keys.items()}
    want_m = {n: (cat("out_m_", ks), cat("out_v_", ks)) for n, ks in keys.items()}
    return d, params, moments, want, want_m


@pytest.mark.parametrize("gt", [False, True], ids=["plain_prune", "cloud"])
@pytest.mark.parametrize("case", ["plain", "scaffold"])
def test_reference_reproduces_the_reference_run(case, gt):
    d, params, moments, want, want_m = _fixture(case, gt)
    args = dict(max_grad=float(d["max_grad"]), min_opacity=float(d["min_opacity"]), extent=float(d["extent"]),
                percent_dense=float(d["percent_dense"]), first_row=int(d["scaffold"]))
    bad = DR.undecided(params["opacity"], params["scaling"], d["in_accum"], d["in_max_radii2D"], **args)
    assert bad.size == 0, bad
    if gt:
        args.update(cloud=d["cloud"], thr=float(d["threshold"]))
    r = DR.densify_ref(params, moments, d["in_accum"], d["in_max_radii2D"], d["normals"], **args)
    c = r["counts"]
    assert c["total"] == want["xyz"].shape[0] and 2 * c["split"] == d["normals"].shape[0]
    assert c["kept"] + c["cloned"] + 2 * r["split_kept"] == c["total"] and c["cloned"] > 0 and c["split"] > 0
    if gt:
        assert r["gt_pruned"] == int(d["gt_pruned"]) > 0 and r["gt_pruned_fixed"] == int(d["gt_pruned_fixed"])
    child = r["child"]
    for name in DR.PARAMS:
        got, ref = r["params"][name].astype(np.float32), want[name]
        rows = ~child if name in ("xyz", "scaling") else np.ones(c["total"], bool)
        np.testing.assert_array_equal(got[rows], ref[rows], err_msg=name)  # row order and copies
        for k in (0, 1):
            np.testing.assert_array_equal(r["moments"][name][k].astype(np.float32), want_m[name][k], err_msg=name)
    ex = np.abs(want["xyz"][child].astype(np.float64) - r["params"]["xyz"][child]) / r["child_bound_xyz"]
    es = np.abs(want["scaling"][child].astype(np.float64) - r["params"]["scaling"][child]) / r["child_bound_scaling"]
    assert ex.max() <= 1.0 and es.max() <= 1.0, (ex.max(), es.max())
    for k in ("out_accum", "out_denom", "out_max_radii2D"):
        assert d[k].shape[0] == c["total"] and not d[k].any()


@pytest.mark.parametrize("name", list(CASES))
def test_case_has_no_undecided_row_and_its_ties_are_the_source_operators(name):
    case = CASES[name]()
    s = case["scalars"]
    args = (s["max_grad"], s["min_opacity"], s["extent"], s["percent_dense"], s["first_row"])
    bad = DR.undecided(case["params"]["opacity"], case["params"]["scaling"], case["accum"], case["max_radii"], *args,
                       exact_ties=case["ties"])
    assert bad.size == 0, (name, bad)
    # deterministic by seed
    again = CASES[name]()
    for k in DR.PARAMS:
        np.testing.assert_array_equal(case["params"][k], again["params"][k])
    np.testing.assert_array_equal(case["accum"], again["accum"])
    clone, split, prune = DR.predicates(case["params"]["opacity"], case["params"]["scaling"], case["accum"],
                                        case["max_radii"], *args)
    for row, want in case["ties"].items():
        assert (bool(clone[row]), bool(split[row]), bool(prune[row])) == tuple(want), (name, row, want)
    f = case["params"]["features"].reshape(-1, 48)
    assert np.array_equal(f.astype(np.int64), 48 * np.arange(f.shape[0])[:, None] + np.arange(48)[None])


def _plan(case):
    return DR.plan(case["params"], case["accum"], case["max_radii"], **EC.run_args(case))


@pytest.mark.parametrize("P", [p for p in EC.SIZES if p >= 255])
def test_sizes_are_mixed(P):
    r = _plan(EC.sizes(P))
    c = r["counts"]
    assert c["cloned"] > 0 and c["split"] > 0 and 0 < c["kept"] < P and r["prune"].any()
    # the apply kernel's groups (widths 3, 48, 1, 3, 4) end inside a 256-lane block, not on one
    assert (c["total"] * np.array([3, 1]) % 256 != 0).all() and c["total"] % 64 != 0 or P == 257
    if P == 257:  # 368 rows: the 48-wide group ends on a block boundary, the others inside one
        assert c["total"] * 48 % 256 == 0 and c["total"] * 3 % 256 != 0


def test_ties_case_populations():
    for case in (EC.ties(), EC.ties(0.05)):
        assert len(case["ties"]) == 32
        p = case["params"]
        tie_rows = np.array(sorted(case["ties"]))
        # the exact values the ties rest on
        assert (p["scaling"][tie_rows] == 0).any() and (p["opacity"][tie_rows] == 0).any()
        assert (case["accum"][tie_rows] == np.float32(0.25)).any()
        assert (case["accum"][tie_rows] == np.nextafter(np.float32(0.25), np.float32(0))).any()
        t = DR.thresholds(**{k: case["scalars"][k] for k in ("max_grad", "min_opacity", "extent", "percent_dense")})
        assert t["max_scale"] == 1.0 and t["max_grad"] == 0.5
        op, c_clone, c_split, smax = DR.quantities(p["opacity"], p["scaling"], case["accum"], case["max_radii"])
        assert (smax[tie_rows] == 1.0).sum() >= 6 and (c_clone[tie_rows] == 0.5).sum() >= 6
        assert (op[tie_rows] == 0.5).sum() >= 8 and (op[tie_rows] == 1.0).sum() >= 12
        ordinary = np.setdiff1d(np.arange(300), tie_rows)
        r = _plan(case)
        assert r["clone"][ordinary].any() and r["split"][ordinary].any() and r["prune"][ordinary].any()
    assert EC.ties()["scalars"]["min_opacity"] == 0.5


def test_overlap_case_populations():
    case = EC.overlap()
    r = _plan(case)
    c = r["counts"]
    assert 0 < r["split_kept"] < c["split"]
    assert (r["clone"] & r["prune"]).sum() > 10 and (r["split"] & r["prune"]).sum() > 10
    kept = np.nonzero(r["split"] & ~r["prune"])[0]
    pruned = np.nonzero(r["split"] & r["prune"])[0]
    between = (pruned > kept.min()) & (pruned < kept.max())
    assert between.sum() > 10
    # so the rank over all split rows and the rank over the kept ones differ on most kept rows
    rank_all = (np.cumsum(r["split"]) - r["split"])[kept]
    assert (rank_all != np.arange(kept.size)).sum() > kept.size // 2


def test_scaffold_case_populations():
    base = _plan(EC.scaffold(0))
    for first in EC.SCAFFOLD_FIRST:
        case = EC.scaffold(first)
        np.testing.assert_array_equal(case["params"]["scaling"], EC.scaffold(0)["params"]["scaling"])
        r = _plan(case)
        lo = slice(0, min(first, EC.SCAFFOLD_P))
        assert not (r["clone"][lo].any() or r["split"][lo].any() or r["prune"][lo].any())
        if first > 1:  # rows that would clone, split and be pruned are shielded
            assert base["clone"][lo].any() and base["split"][lo].any() and base["prune"][lo].any()
        if first == 1:
            assert base["clone"][0]
        if first >= EC.SCAFFOLD_P:
            assert r["counts"] == dict(kept=EC.SCAFFOLD_P, cloned=0, split=0, total=EC.SCAFFOLD_P)


def test_extreme_case_outcomes():
    P = 300
    want = {"nothing": dict(kept=P, cloned=0, split=0, total=P), "all_pruned": dict(kept=0, cloned=0, split=0, total=0),
            "all_split": dict(kept=0, cloned=0, split=P, total=2 * P),
            "all_cloned": dict(kept=P, cloned=P, split=0, total=2 * P), "empty": dict(kept=0, cloned=0, split=0, total=0)}
    for which in EC.EXTREMES:
        assert _plan(EC.extremes(which))["counts"] == want[which], which
    assert EC.extremes("empty")["params"]["xyz"].shape == (0, 3)


def test_accumulator_case_outcomes():
    case = EC.accumulator()
    r = _plan(case)
    for row, want in EC.accumulator_expected().items():
        assert (bool(r["clone"][row]), bool(r["split"][row]), bool(r["prune"][row])) == want, row
    a = case["accum"][:, 0]
    assert np.isnan(a).sum() == 3 and np.isinf(a).sum() == 5 and (a < 0).sum() == 6
    assert (case["max_radii"] == 0).sum() >= 4 and (np.abs(a[a != 0]) < 1e-38).any()
    assert r["clone"][60] and not r["split"][61] and r["split"][31]  # |g| clones; g does not split; +Inf does


def test_zero_threshold_case_selects_the_zeroed_nan_rows():
    case = EC.zero_threshold()
    r = _plan(case)
    nan = np.isnan(case["accum"][:, 0])
    zero = case["accum"][:, 0] == 0
    assert nan.sum() == 14 and zero.sum() == 14
    sel = r["clone"] | r["split"]
    assert (sel & nan).sum() >= 8 and (sel & zero).sum() >= 8 and (r["clone"] & nan).any() and (r["split"] & nan).any()
    op = DR.quantities(case["params"]["opacity"], case["params"]["scaling"], case["accum"], case["max_radii"])[0]
    assert np.array_equal(sel, op > DR.OP_ELIGIBLE)  # max_grad = 0 selects every eligible row


def test_quaternion_case_populations():
    case = EC.quaternions()
    r, _ = EC.reference(case)
    assert r["counts"] == dict(kept=0, cloned=0, split=64, total=128)
    n = np.linalg.norm(case["params"]["rotation"].astype(np.float64), axis=1)
    assert n[EC.QUAT_ZERO_ROW] == 0 and n[n > 0].min() < 2e-3 and n.max() > 500
    nan_rows = np.isnan(r["params"]["xyz"]).any(axis=1)
    assert np.array_equal(np.nonzero(nan_rows)[0], [EC.QUAT_ZERO_ROW, 64 + EC.QUAT_ZERO_ROW])
    assert np.isnan(r["params"]["xyz"][nan_rows]).all() and np.isfinite(r["params"]["scaling"]).all()
    s = case["params"]["scaling"]
    assert s.min() < -11 and s.max() > 3 and np.abs(case["params"]["xyz"]).max() > 3e3


def test_no_state_cases():
    assert EC.no_state("none")["moments"] == {} and EC.no_state("none")["no_state"]
    assert set(EC.no_state("some")["moments"]) == {"xyz", "opacity"}
    r, _ = EC.reference(EC.no_state("some"))
    assert set(r["moments"]) == {"xyz", "opacity"} and r["counts"]["cloned"] > 0 and r["counts"]["split"] > 0


def test_cloud_case_populations():
    import gt_ref
    case = EC.cloud()
    r = _plan(case)
    first = case["scalars"]["first_row"]
    xyz = case["params"]["xyz"]
    far_all = gt_ref.far_mask(xyz, case["cloud"], case["thr"])  # without the skips
    inside = gt_ref.inside_bounds(xyz, case["cloud"])
    clone, split, prune = r["clone"], r["split"], r["prune"]
    assert first > 0
    assert (far_all & ~split & ~prune & ~clone).any()          # far and kept-as-was: the old row goes
    assert (far_all & clone & ~prune).any()                    # far and cloned: both go
    assert (far_all & split).any() and not r["far"][split].any()  # far and split: not tested
    assert (far_all & prune).any() and not r["far"][prune].any()  # far and opacity-pruned: not counted
    assert far_all[:first].any() and r["gt_pruned_fixed"] == int(far_all[:first].sum()) > 0
    assert (~inside).sum() > 100 and not far_all[~inside].any()
    assert r["gt_pruned"] == int((r["far"] & ~split & ~prune).sum() + (r["far"] & clone & ~prune).sum()) > 0
    assert r["gt_pruned"] < int(far_all.sum()) + int((far_all & clone).sum())
    # every checked row's squared distance is clear of thr^2
    d2 = gt_ref.min_d2(xyz[inside], case["cloud"]).astype(np.float64)
    assert (np.abs(d2 / case["thr"] ** 2 - 1.0) > 0.5).all()
    # without the cloud the same rows survive
    plain = DR.plan(case["params"], case["accum"], case["max_radii"], **dict(EC.run_args(case), cloud=None, thr=None))
    assert plain["counts"]["total"] == r["counts"]["total"] + r["gt_pruned"]


def test_two_events_in_a_row_have_inputs():
    case = EC.sizes(257)
    r, _ = EC.reference(case)
    p2 = {k: v.astype(np.float32) for k, v in r["params"].items()}
    accum, maxr = EC.second_stats(p2, seed=5)
    s = case["scalars"]
    assert DR.undecided(p2["opacity"], p2["scaling"], accum, maxr, s["max_grad"], s["min_opacity"], s["extent"],
                        s["percent_dense"], 0).size == 0
    c = DR.plan(p2, accum, maxr, **EC.run_args(case))["counts"]
    assert c["cloned"] > 0 and c["split"] > 0 and c["kept"] < p2["xyz"].shape[0]


def test_larger_random_state_is_almost_all_decided():
    """tests/test_gpu_densify.py's 20 011-row state: fewer than 0.1 % of its rows are undecided, so
    the comparison with densify_ref on the decided rows covers nearly all of it."""
    a = EC.state_arrays(20_011, 3)[0]
    bad = DR.undecided(a["opacity_raw"], a["scaling_raw"], a["accum"], a["max_radii"], *EC.STATE_ARGS)
    assert bad.size < 0.001 * 20_011, bad.size


def test_stats_inputs_hold_every_kind():
    for P in EC.STATS_SIZES:
        d = EC.stats_inputs(P)
        mr, acc, den = DR.stats_ref(d["radii"], d["grad2d"], d["max_r"], d["accum"], d["denom"])
        hidden = d["radii"] <= 0
        assert np.array_equal(acc[hidden], d["accum"][hidden].astype(np.float64), equal_nan=True)
        assert np.array_equal(den[~hidden], d["denom"][~hidden] + 1.0) and np.isnan(acc).any()
        if P > 1:
            for k in range(9):
                assert (d["kinds"] == k).any()
            assert np.isnan(acc[np.isin(d["kinds"], (3, 4, 5))]).all()  # torch.max propagates NaN, both ways
            assert np.isinf(acc[d["kinds"] == 6]).all() and (acc[d["kinds"] == 2] == 5.0).all()
            assert not np.isnan(acc[np.isin(d["kinds"], (2, 6, 7, 8))]).any()
