"""CPU tests of the hierarchy-cut edge cases (tests/cut_cases.py) and their float64 reference
(tests/cut_ref.py): the reference against the reference-generated fixture and against torch float64
autograd of the reference's formulation, the condition that no case holds a row float32 could decide
either way, what each case is for, and a float32 evaluation of the same formulas against the bars of
tests/test_gpu_cut_edges.py -- which also measures the constants of the raw form's bars and writes them
to profiles/r19_cut_edge_margins.jsonl."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import cut_cases as C
import cut_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "render_post.npz")
MARGINS = os.path.join(REPO, "profiles", "r19_cut_edge_margins.jsonl")
ACTS = {"act": (0,), "raw": (R.SIGMOID, R.ABS)}
CASES = [(n, f) for n in C.NAMES for f in C.FORMS]


def test_reference_reproduces_the_reference_fixture():
    f = np.load(GOLD)
    ri = f["render_indices"]
    c = dict(N=f["xyz"].shape[0], M=f["features"].shape[1], S=int(f["skybox"]), ri=ri, pi=f["parent_indices"][:len(ri)],
             w=f["interpolation_weights"][:len(ri)], **{k: f[k] for k in R.FIELDS})
    outs, _ = R.forward(c, 0)
    for name in R.OUTS:
        np.testing.assert_allclose(outs[name], f["out_" + name], rtol=0, atol=1e-6, err_msg=name)


def _blend_activated(x, ri, pi, w, S):
    """render_post's gather over activated values (tests/test_gpu_hier.py's formulation), float64."""
    N = x[0].shape[0]
    r, p = ri.long(), pi.long() % N
    t = w[:len(ri)].double()[:, None]
    par = x[2][p]
    sign = torch.where((x[2][r] * par).sum(1, keepdim=True) < 0, -1.0, 1.0).double()
    outs = [t * x[0][r] + (1 - t) * x[0][p], t * x[1][r] + (1 - t) * x[1][p], t * x[2][r] + (1 - t) * par * sign,
            t * x[3][r] + (1 - t) * x[3][p], t[:, :, None] * x[4][r] + (1 - t[:, :, None]) * x[4][p]]
    sk = torch.arange(N - S, N)
    return [torch.cat([o, xx[sk]]) for o, xx in zip(outs, x)]


@pytest.mark.parametrize("name,form", CASES)
def test_reference_equals_torch_float64_autograd(name, form):
    from test_gpu_post import _reference_blend
    c = C.case(name, form)
    ups = C.upstreams(c)
    ri, pi, w = torch.tensor(c["ri"]), torch.tensor(c["pi"]), torch.tensor(c["w"])
    for act in ACTS[form]:
        x = [torch.tensor(c[k], dtype=torch.float64, requires_grad=True) for k in R.FIELDS]
        want = _blend_activated(x, ri, pi, w, c["S"]) if act == 0 else _reference_blend(x, ri, pi, w, c["S"], act)
        outs, scales = R.forward(c, act)
        for o, k in zip(want, R.OUTS):
            assert np.all(np.abs(o.detach().numpy() - outs[k]) <= 1e-13 * scales[k]), (k, act)
        sum((o * torch.tensor(u, dtype=torch.float64)).sum() for o, u in zip(want, ups)).backward()
        res = R.backward(c, ups, act)
        for xx, k in zip(x, R.FIELDS):
            val, size, cnt = res[k]
            assert np.all(np.abs(xx.grad.numpy() - val) <= 1e-12 * size), (k, act)
            assert np.all(val[cnt == 0] == 0) and np.all(size[cnt == 0] == 0), k


def _f32_dots(c, act):
    """The rotation dot in float32, summed left to right and right to left."""
    ch, pa, _, _ = R.rows(c)
    q = R.activate(c, act, np.float32)[2]
    p = q[ch] * q[pa]
    return ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3], ((p[:, 3] + p[:, 2]) + p[:, 1]) + p[:, 0]


@pytest.mark.parametrize("name,form", CASES)
def test_no_row_float32_could_decide_either_way(name, form):
    """The sign of the rotation dot: a float32 dot of four products is within 4 * 2^-24 * sum |terms| of
    the exact one and the normalisation of the raw form adds a few ulp to each factor, so a row whose
    |dot| is at least 64 * 2^-24 * sum |q_c,k q_p,k| has its sign in any float32 evaluation; a tie row's
    float32 dot is exactly 0 in both summation orders.  F.normalize's clamp: no norm within 1e-4 relative
    of eps other than 0.  sgn of the abs opacity: the stored values are float32, exact."""
    c = C.case(name, form)
    R_ = len(c["ri"])
    for act in ACTS[form]:
        dot, mag = R.rotation_dots(c, act)
        a, b = _f32_dots(c, act)
        tie = np.concatenate([c["tie"], np.zeros(c["S"], bool)])
        assert np.all(a[tie] == 0) and np.all(b[tie] == 0) and np.all(dot[tie] == 0)
        free = ~tie
        free[R_:] = False  # a skybox copy takes no sign
        assert np.all(np.abs(dot[free]) >= 64 * R.U * mag[free]), (c["name"], np.flatnonzero(free & (np.abs(dot) < 64 * R.U * mag)))
        assert np.array_equal(a[free] < 0, dot[free] < 0) and np.array_equal(b[free] < 0, dot[free] < 0)
    if form == "raw":
        n = np.linalg.norm(c["rotation"].astype(np.float64), axis=1)
        assert np.all((n == 0) | (np.abs(n / R.NORM_EPS - 1) >= 1e-4))


def test_sized_cases_of_the_gpu_tests_meet_the_condition():
    from test_gpu_cut_edges import sized_cases_used
    seen = 0
    for c in sized_cases_used():
        assert c["unique"] and R.meets_unique_precondition(c), c["name"]
        n = len(c["ri"])
        for act in ACTS[c["form"]]:
            dot, mag = R.rotation_dots(c, act)
            assert np.all(np.abs(dot[:n]) >= 64 * R.U * mag[:n]), c["name"]
        seen += 1
    assert seen >= 60


def _crossing(runs, B):
    return [(s, n) for s, n in runs if (s + n - 1) // B > s // B]


def test_cases_hold_what_they_are_for():
    for c in C.all_cases():
        assert c["N"] <= 3100 and c["unique"] == R.meets_unique_precondition(c), c["name"]
        assert np.all(np.isfinite(np.concatenate([c[k].ravel() for k in R.FIELDS])))
    for form in C.FORMS:
        runs = C.case("runs", form)["runs"]
        lengths = {n for _, n in runs}
        assert set(C.RUN_LENGTHS) <= lengths
        for B in (16, 64, 256):
            assert _crossing(runs, B), B
        for L in C.RUN_LENGTHS[:-1]:  # on and next to the 16- and 64-row edges, starting and ending
            for B in (16, 64):
                at = {(s % B, (s + n) % B) for s, n in runs if n == L}
                assert {B - 1, 0, 1} <= {a for a, _ in at} | {b for _, b in at}, (L, B, at)
        assert {s % 256 for s, n in runs if n in (17, 64, 65)} >= {255, 0, 1}
        assert any(s < 256 * k and s + n >= 256 * (k + 1) for s, n in runs for k in range(1, 12))  # a whole block
        assert C.case("one_parent", form)["runs"] == [(0, 333)]
        # A A B A with B on a 16-row and on a 64-row edge
        a = C.case("aaba", form)
        p = a["pi"]
        for b in (2, 16, 64):
            assert p[b - 2] == p[b - 1] == p[b + 1] != p[b], b
        assert p[-4] == p[-2] != p[-3] == p[-1]
        s = C.case("split_by_skybox", form)
        assert s["runs"][-1][1] == 25 and len(s["ri"]) % 16 and len(s["ri"]) % 64 and s["S"] > 16
        r = C.case("roots_w1", form)
        assert (r["pi"] < 0).sum() >= 6 and np.all(r["w"][r["pi"] < 0] == 1) and r["S"] > 0 and r["unique"]
        for name in C.ACCUMULATING:
            assert not C.case(name, form)["unique"], name
        for name, S in (("roots_w025_S0", 0), ("roots_w025_S", 4)):
            r = C.case(name, form)
            assert r["S"] == S and (r["pi"] < 0).sum() >= 4 and np.all(r["w"][r["pi"] < 0] == np.float32(0.25))
        k = C.case("child_is_parent", form)
        assert len(np.intersect1d(k["ri"], k["pi"])) > 30
        k = C.case("p_eq_c", form)
        assert (k["ri"] == k["pi"]).sum() >= 50
        k = C.case("child_twice", form)
        assert len(np.unique(k["ri"])) <= len(k["ri"]) - 99 and k["ri"].max() == k["N"] - 1
        t = C.case("ties", form)
        assert t["tie"].sum() >= 40 and (~t["tie"]).sum() >= 20 and t["unique"]
        assert np.all(t["w"][t["tie"]] != 1)
        tied_runs = [(s, n) for s, n in t["runs"] if n >= 3 and t["tie"][s:s + n].all()]
        assert tied_runs  # tie siblings under one parent: the unique backward's scan sums them
        for act in ACTS[form]:
            dot, _ = R.rotation_dots(t, act)
            free = dot[:len(t["ri"])][~t["tie"]]
            assert (free > 0).any() and (free < 0).any()
            exact = dot[:len(t["ri"])][:5 * len(C.ACT_PAIRS if form == "act" else C.RAW_PAIRS)]
            assert set(np.unique(exact)) >= ({-.25, 0, .25} if form == "act" else {-1, -.5, 0, .5, 1})
        w = C.case("weights", form)["w"]
        assert set(np.float32(C.WEIGHTS)) == set(w) and min(np.bincount(np.searchsorted(np.sort(np.float32(C.WEIGHTS)), w))) >= 10
        o = C.case("opacity_edges", form)
        for rows_ in (o["ri"], np.unique(o["pi"]), np.arange(o["N"] - o["S"], o["N"])):
            got = {(float(v), bool(np.signbit(v))) for v in o["opacity"][rows_, 0]}
            assert got == {(float(np.float32(v)), bool(np.signbit(v))) for v in C.OPACITY_EDGES}
    raw = C.case("ties", "raw")
    n = np.linalg.norm(raw["rotation"].astype(np.float64), axis=1)
    for want in C.QUAT_NORMS:
        assert (np.abs(n - want) <= 1e-6 * want).sum() >= 3, want
    assert C.case("runs", "raw")["scaling"].min() < -19 and C.case("runs", "raw")["scaling"].max() > 2.9
    s = C.sized_case(0, 5, spare=0)
    assert s["N"] == s["S"] == 5 and len(s["ri"]) == 0
    assert (C.sized_case(10, 3)["N"] - 3) % 2 or (C.sized_case(10, 3, spare=4)["N"] - 3) % 2


def _ratio(err, unit):
    """max |err| / unit, where a zero unit asks for a zero error."""
    err, unit = np.abs(err).astype(np.float64), unit.astype(np.float64)
    assert np.all(err[unit == 0] == 0)
    return float((err[unit > 0] / unit[unit > 0]).max()) if (unit > 0).any() else 0.0


def _measure(c, act):
    """{field: ratio} of the float32 evaluation against float64, in the units of the bars."""
    ups = C.upstreams(c)
    o64, scales = R.forward(c, act)
    o32, _ = R.forward(c, act, np.float32)
    out = {k: _ratio(o32[k] - o64[k], R.U * scales[k]) for k in R.OUTS}
    g64, g32 = R.backward(c, ups, act), R.backward(c, ups, act, np.float32)
    for k in R.FIELDS:
        assert np.all(g32[k][0][g64[k][2] == 0] == 0)
        out["grad_" + k] = _ratio(g32[k][0] - g64[k][0], R.grad_bar(g64, k))
    return out


def test_float32_evaluation_stays_inside_the_bars():
    """The bars against the reference alone.  Activated form: 4 units forward, 1 unit backward (derived
    in tests/cut_ref.py).  Raw form: the largest ratio of each field over the cases is written to
    profiles/r19_cut_edge_margins.jsonl (kind cpu_f32); the GPU test's bar is 4x it, the margin
    profiles/r12_shape_margins.jsonl gives a device libm over the host's, and no less than the derived
    bar of the activated form (the activations add roundings, they remove none).  The lines the GPU test
    recorded (its own ratios, for the record) are kept."""
    worst = {}
    for c in C.all_cases():
        for act in ACTS[c["form"]]:
            for k, r in _measure(c, act).items():
                if act == 0:
                    assert r <= (1.0 if k.startswith("grad_") else 4.0), (c["name"], k, r)
                key = (act, k)
                if r >= worst.get(key, (-1.0, ""))[0]:
                    worst[key] = (r, c["name"])
    kept = []
    if os.path.exists(MARGINS):
        with open(MARGINS) as f:
            kept = [ln for ln in f if ln.strip() and json.loads(ln).get("kind") != "cpu_f32"]
    os.makedirs(os.path.dirname(MARGINS), exist_ok=True)
    with open(MARGINS, "w") as f:
        for (act, k), (r, name) in sorted(worst.items()):
            f.write(json.dumps({"kind": "cpu_f32", "act": act, "field": k, "ratio": r, "case": name}) + "\n")
        f.writelines(kept)
    for (act, k), (r, name) in worst.items():
        assert np.isfinite(r) and r < 64, (act, k, r, name)  # a bar of hundreds of units would hold nothing


def test_weight_rule_is_exact_on_the_hand_built_hierarchies():
    """Every intermediate of the float64 rule is a float32 number on every query, so float32 decides and
    computes the same; the C restatement agrees exactly; every branch of the rule is taken."""
    import gs_oracle as O
    seen = set()
    for name, nodes, boxes, v, target in C.weight_queries():
        assert 3 <= len(nodes) <= 300
        idx = np.arange(len(nodes), dtype=np.int32)
        w, kids, exact = R.interpolation_weights(idx, target, nodes, boxes, v)
        assert exact.all(), name
        ow, ok = O.interpolation_weights(idx, np.float32(target), nodes, boxes, np.asarray(v, np.float32))
        assert np.array_equal(ow.astype(np.float64), w) and np.array_equal(ok, kids), name
        assert w[0] == 1 and kids[0] == 1 and np.all(kids[1:] == len(nodes) - 1)
        seen |= {("t", float(t)) for t in w}
        sp = R.node_size(boxes[0], v)
        seen.add(("sp", "inside" if sp == R.FLT_MAX else "eq" if sp == 2 * np.float32(target) else
                  "above" if sp > 2 * np.float32(target) else "below"))
    assert {("t", 0.0), ("t", 1.0), ("t", 0.5), ("t", 0.75), ("t", 1 - 2.0 ** -23)} <= seen
    assert {("sp", k) for k in ("inside", "eq", "above", "below")} <= seen
