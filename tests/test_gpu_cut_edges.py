"""GPU tests of the hierarchy-cut blend (csrc/hier.hip: gs_train.hier.interpolate_cut, gs_train.post.
interpolate_cut_act with both opacity activations and both backward modes, the scalar SH path, gsr_zero_grad_rows)
and of the blend weight (csrc/lod.hip get_interpolation_weights) on the inputs of tests/cut_cases.py, against
the float64 reference tests/cut_ref.py, per element.

Bars (units: 2^-24 * fwd_scale forward, (grad_cnt + 2) * 2^-24 * grad_abs backward; tests/cut_ref.py):
activated form 4 units forward and 1 unit backward, both derived; raw form 4x the ratio a float32 evaluation
of the same formulas reaches on the host (profiles/r19_cut_edge_margins.jsonl, kind cpu_f32, written by
tests/test_cut_cases_cpu.py) and no less than the activated form's.  An element no row contributes to must
be exactly zero.  The ratios the GPU reaches go to $GSR_PARITY_RECORD (for the record; no bar is set from
them).  Mutants caught: profiles/r19_cut_edge_mutation_check.txt."""
from __future__ import annotations

import functools
import json
import os

import numpy as np
import pytest
import torch

import cut_cases as C
import cut_ref as R
from helpers import record_margins

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGINS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                       "r19_cut_edge_margins.jsonl")
UNIQUE = 0x100
ALL = (0, 1, 2, 3, 4)


@functools.lru_cache(maxsize=None)
def _constants():
    """{(act, field): units}"""
    k = {(0, f): 4.0 for f in R.OUTS}
    k.update({(0, "grad_" + f): 1.0 for f in R.FIELDS})
    with open(MARGINS) as f:
        rows = [json.loads(ln) for ln in f if ln.strip()]
    for r in rows:
        if r.get("kind") == "cpu_f32" and r["act"] != 0:
            k[(r["act"], r["field"])] = max(k[(0, r["field"])], 4.0 * r["ratio"])
    assert len(k) == 30, "profiles/r19_cut_edge_margins.jsonl lacks cpu_f32 lines"
    return k


_REFS = {}


def _reference(c, act, subset=ALL, seed=0):
    key = (c["name"], act, subset, seed)
    if key not in _REFS:
        ups = C.upstreams(c, seed, subset)
        outs, scales = R.forward(c, act)
        _REFS[key] = (ups, outs, scales, R.backward(c, ups, act))
    return _REFS[key]


def _dev(a, dtype=None):
    return torch.tensor(np.asarray(a), device=DEV, dtype=dtype)


def _wrappers(c, act, unique, ups):
    """Through gs_train.hier.interpolate_cut (act 0) or gs_train.post.interpolate_cut_act -> numpy outs, grads."""
    from gs_train.hier import interpolate_cut
    from gs_train.post import interpolate_cut_act
    xs = [_dev(c[k]).requires_grad_(True) for k in R.FIELDS]
    idx = (_dev(c["ri"]), _dev(c["pi"]), _dev(c["w"]))
    if act == 0:
        outs = interpolate_cut(*xs, *idx, c["S"])
    else:
        outs = interpolate_cut_act(*xs, *idx, c["S"], opacity_act=act, unique_children=unique)
    given = [k for k in range(5) if ups[k] is not None]
    torch.autograd.backward([outs[k] for k in given], [_dev(ups[k]) for k in given])
    torch.cuda.synchronize()
    return [o.detach().cpu().numpy() for o in outs], [x.grad.cpu().numpy() for x in xs]


def _view(a, off, fill=None):
    """A contiguous device tensor of a's shape that starts `off` floats into a larger buffer."""
    a = np.asarray(a, np.float32)
    buf = torch.full((a.size + off + 4,), float("nan") if fill is None else fill, device=DEV)
    v = buf[off:off + a.size].view(a.shape)
    if fill is None:
        v.copy_(_dev(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


def _direct(c, act, unique, ups, sh_off=0, M=None, S=None, rot_off=0, sentinel=float("nan")):
    """Through the C ABI (gs_train._native.lib).  sh_off: the four SH arrays start that many floats past
    a 16-byte boundary.  -> (rc forward, rc backward, numpy outs, numpy grads)."""
    from gs_train._native import lib, ptr, stream
    L = lib()
    N, M = c["N"], c["M"] if M is None else M
    S = c["S"] if S is None else S
    R_ = len(c["ri"])
    rows = R_ + S
    ri, pi, w = _dev(c["ri"]), _dev(c["pi"]), _dev(c["w"])
    ins = [_dev(c["xyz"]), _dev(c["scaling"]), _view(c["rotation"], rot_off), _dev(c["opacity"]),
           _view(c["features"], sh_off)]
    shapes = [(3,), (3,), (4,), (1,), c["features"].shape[1:]]
    outs = [_view(np.zeros((rows,) + s, np.float32), sh_off if k == 4 else 0, fill=sentinel) for k, s in enumerate(shapes)]
    st = stream(torch.device(DEV))
    head = (N, M, R_, S, ptr(ri), ptr(pi), ptr(w))
    if act == 0:
        rf = L.gsr_interpolate_cut_forward(*head, *[ptr(t) for t in ins], *[ptr(t) for t in outs], st)
    else:
        rf = L.gsr_interpolate_cut_forward_act(*head, *[ptr(t) for t in ins], act, *[ptr(t) for t in outs], st)
    g = [_view(np.zeros((rows,) + s, np.float32) if ups is None or ups[k] is None else ups[k], sh_off if k == 4 else 0)
         for k, s in enumerate(shapes)]
    grads = [_view(np.zeros((N,) + s, np.float32), sh_off if k == 4 else 0, fill=0.0) for k, s in enumerate(shapes)]
    if act == 0:
        rb = L.gsr_interpolate_cut_backward(*head, ptr(ins[2]), *[ptr(t) for t in g], *[ptr(t) for t in grads], st)
    else:
        rb = L.gsr_interpolate_cut_backward_act(*head, ptr(ins[1]), ptr(ins[2]), ptr(ins[3]),
                                                act | (UNIQUE if unique else 0), *[ptr(t) for t in g],
                                                *[ptr(t) for t in grads], st)
    torch.cuda.synchronize()
    return rf, rb, [o.cpu().numpy() for o in outs], [x.cpu().numpy() for x in grads]


def _ratio(err, unit):
    ok = unit > 0
    return float((err[ok] / unit[ok]).max()) if ok.any() else 0.0


def _compare(c, act, outs, grads, tag, subset=ALL):
    """Every output and gradient element against the reference; returns the measured ratios."""
    K = _constants()
    ups, ro, scales, rg = _reference(c, act, subset)
    seen = {}
    for k, name in enumerate(R.OUTS):
        assert outs[k].shape == ro[name].shape, (tag, name)
        err, unit = np.abs(outs[k].astype(np.float64) - ro[name]), R.U * scales[name]
        seen[name] = _ratio(err, unit)
        bad = ~(err <= K[(act, name)] * unit)
        assert not bad.any(), (tag, name, int(bad.sum()), np.argwhere(bad)[0].tolist(), seen[name])
    for k, field in enumerate(R.FIELDS):
        val, _, cnt = rg[field]
        assert grads[k].shape == val.shape, (tag, field)
        err, unit = np.abs(grads[k].astype(np.float64) - val), R.grad_bar(rg, field)
        seen["grad_" + field] = _ratio(err, unit)
        bad = ~(err <= K[(act, "grad_" + field)] * unit)
        assert not bad.any(), (tag, field, int(bad.sum()), np.argwhere(bad)[0].tolist(), seen["grad_" + field])
        assert not grads[k][cnt == 0].any(), (tag, field, "a row nothing contributes to")
    record_margins(f"cut_edges/{tag}", **seen)
    return seen


def _modes(c):
    """(act, unique) of every entry point the case may go through."""
    if c["form"] == "act":
        return [(0, False)]
    return [(a, u) for a in (R.SIGMOID, R.ABS) for u in ((False, True) if c["unique"] else (False,))]


def _run_all_modes(c, run=_wrappers, subset=ALL):
    grads = {}
    for act, unique in _modes(c):
        ups = _reference(c, act, subset)[0]
        outs, g = run(c, act, unique, ups)
        _compare(c, act, outs, g, f"{c['name']}/act{act}{'u' if unique else ''}", subset)
        grads[(act, unique)] = g
    # a cut's child rows are written: bit-equal to an atomic add into a zero row
    child = c["ri"].astype(np.int64)
    for (act, unique), g in grads.items():
        if unique:
            for a, b in zip(g, grads[(act, False)]):
                assert np.array_equal(a[child], b[child]), (c["name"], act)
    return grads


@pytest.mark.parametrize("form", C.FORMS)
@pytest.mark.parametrize("name", C.NAMES)
def test_named_cases(name, form):
    _run_all_modes(C.case(name, form))


SIZES = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025)
ROW_COUNTS = [(0, 5, 3), (0, 40, 0), (100, 7, 3), (100, 7, 4), (1, 0, 0)]  # R, S, spare rows
SH_PATHS = [(1, 0), (4, 0), (9, 0), (16, 1)]  # M, floats past a 16-byte boundary


def _sky(rows, sky):
    return max(1, rows // 3) if sky else 0


def sized_cases_used():
    """Every cut_cases.sized_case of this file (tests/test_cut_cases_cpu.py holds them to the cases'
    condition too)."""
    for form in C.FORMS:
        for rows in SIZES:
            for sky in (False, True):
                yield C.sized_case(rows - _sky(rows, sky), _sky(rows, sky), form=form)
        for R_, S, spare in ROW_COUNTS:
            yield C.sized_case(R_, S, form=form, spare=spare)
        for M, _ in SH_PATHS:
            yield C.sized_case(300, 21, M=M, form=form)
        yield C.sized_case(40, 4, form=form)


@pytest.mark.parametrize("sky", [False, True])
@pytest.mark.parametrize("rows", SIZES)
def test_sizes(rows, sky):
    """R + S on and next to a wave, a block and the 16-row SH run, without a skybox and with the last
    third of the rows (at least one: R = 0 at one row) coming from it."""
    S = _sky(rows, sky)
    for form in C.FORMS:
        c = C.sized_case(rows - S, S, form=form)
        assert len(c["ri"]) + c["S"] == rows
        _run_all_modes(c)


@pytest.mark.parametrize("R_,S,spare", ROW_COUNTS)
def test_further_row_counts(R_, S, spare):
    """Nothing rendered, S = N, N - S odd and even, one row in all."""
    for form in C.FORMS:
        _run_all_modes(C.sized_case(R_, S, form=form, spare=spare))
    c = C.sized_case(R_, S, spare=spare)
    assert (R_, S, spare) != (0, 40, 0) or c["N"] == c["S"]
    assert {(C.sized_case(100, 7, spare=k)["N"] - 7) % 2 for k in (3, 4)} == {0, 1}


@pytest.mark.parametrize("M,off", SH_PATHS)
def test_scalar_sh_path(M, off):
    """M < 16, and M = 16 with every SH pointer 4 bytes past a 16-byte boundary: the per-row loops of the
    forward and of both backward modes, through the C ABI; M < 16 through the wrappers too."""
    for form in C.FORMS:
        c = C.sized_case(300, 21, M=M, form=form)

        def run(c, act, unique, ups):
            rf, rb, outs, grads = _direct(c, act, unique, ups, sh_off=off)
            assert rf == 0 and rb == 0
            return outs, grads

        _run_all_modes(c, run)
        if not off:
            _run_all_modes(c)


def test_tie_rows_take_the_parent_with_sign_plus_one():
    """Rows whose rotation dot is exactly 0: the parent enters with +1.  Where every step is exact (the
    activated form; the forward of the raw form on quaternions with power-of-two norms) the float32 value
    is asked for bit by bit; elsewhere the bar holds for +1 and could not hold for -1."""
    K = _constants()
    for form in C.FORMS:
        c = C.case("ties", form)
        n = len(c["ri"]) - c.get("norm_rows", 0)  # rows built from the exact pairs
        tie = np.flatnonzero(c["tie"][:n])
        own = tie[tie < 5 * len(C.ACT_PAIRS if form == "act" else C.RAW_PAIRS)]  # a parent of their own
        ch, pa, t, _ = R.rows(c)
        for (act, unique), grads in _run_all_modes(c).items():
            ups, ro, _, rg = _reference(c, act)
            outs, _ = _wrappers(c, act, unique, ups)
            q = R.activate(c, act, np.float32)[2]
            u = np.float32(1) - t
            plus = t[tie, None] * q[ch[tie]] + u[tie, None] * q[pa[tie]]
            minus = t[tie, None] * q[ch[tie]] - u[tie, None] * q[pa[tie]]
            assert np.array_equal(outs[2][tie], plus), (form, act)
            assert (np.abs(plus - minus).max(1) > 0).sum() >= 30  # the rows where the sign shows
            # backward: each of these parents has the one contribution (1 - t) g, or F.normalize's
            # backward of it
            p = pa[own]
            assert len(np.unique(p)) == len(p)
            got, (val, size, cnt) = grads[2][p], rg["rotation"]
            if act == 0:
                assert np.array_equal(got, u[own, None] * ups[2][own]), form
            bar = K[(act, "grad_rotation")] * R.grad_bar(rg, "rotation")[p]
            assert np.all(np.abs(got - val[p]) <= bar)
            shows = np.abs(val[p]).max(1) > 2 * bar.max(1)
            assert shows.sum() >= 30 and np.all(np.abs(got + val[p]).max(1)[shows] > bar.max(1)[shows])


@pytest.mark.parametrize("subset", [(2,), (0, 4), (1, 3), (4,)])
def test_upstream_gradients_for_some_outputs_only(subset):
    """The outputs without an upstream gradient reach backward as None."""
    for form in C.FORMS:
        for name in ("aaba", "roots_w1"):
            _run_all_modes(C.case(name, form), subset=subset)


def test_argument_checks_return_an_error_and_launch_nothing():
    from diff_gaussian_rasterization import _lib
    from gs_train.hier import interpolate_cut
    from gs_train.post import interpolate_cut_act
    c = C.sized_case(40, 4, form="raw")
    wide = dict(c, features=np.zeros((c["N"], 17, 3), np.float32), M=17)
    none = dict(c, features=np.zeros((c["N"], 0, 3), np.float32), M=0)
    for what, cc, act, kw in (("S > N", c, 0, dict(S=c["N"] + 1)), ("S > N", c, 2, dict(S=c["N"] + 1)),
                              ("M = 17", wide, 0, {}), ("M = 17", wide, 1, {}), ("M = 0", none, 0, {}),
                              ("M = 0", none, 2, {}), ("rotations", c, 0, dict(rot_off=1)),
                              ("rotations", c, 2, dict(rot_off=1)), ("identity", c, -1, {})):
        if act < 0:  # the _act entry points with GSR_OPACITY_IDENTITY
            rf, rb, outs, grads = _direct_act_identity(cc)
        else:
            rf, rb, outs, grads = _direct(cc, act, False, None, sentinel=-7.0, **kw)
        assert rf != 0 and rb != 0, what
        assert b"gsr_interpolate_cut" in _lib.load().gsr_last_error(), what
        assert all(np.all(o == -7.0) for o in outs) and not any(g.any() for g in grads), what
    xs = [_dev(c[k]) for k in R.FIELDS]
    idx = (_dev(c["ri"]), _dev(c["pi"]), _dev(c["w"]))
    with pytest.raises(RuntimeError, match="opacity_act"):
        interpolate_cut_act(*xs, *idx, c["S"], opacity_act=0)
    with pytest.raises(RuntimeError, match="bad sizes"):
        interpolate_cut(*xs[:4], _dev(wide["features"]), *idx, c["S"])
    with pytest.raises(RuntimeError, match="bad sizes"):
        interpolate_cut_act(*xs, *idx, c["N"] + 1)


def _direct_act_identity(c):
    """_direct's _act calls with opacity_act = GSR_OPACITY_IDENTITY (0), which _direct reads as the
    activated form."""
    from gs_train._native import lib, ptr, stream
    L = lib()
    rows = len(c["ri"]) + c["S"]
    ri, pi, w = _dev(c["ri"]), _dev(c["pi"]), _dev(c["w"])
    ins = [_dev(c[k]) for k in R.FIELDS]
    outs = [torch.full((rows,) + t.shape[1:], -7.0, device=DEV) for t in ins]
    g = [torch.ones((rows,) + t.shape[1:], device=DEV) for t in ins]
    grads = [torch.zeros_like(t) for t in ins]
    st = stream(torch.device(DEV))
    head = (c["N"], c["M"], len(c["ri"]), c["S"], ptr(ri), ptr(pi), ptr(w))
    rf = L.gsr_interpolate_cut_forward_act(*head, *[ptr(t) for t in ins], 0, *[ptr(t) for t in outs], st)
    rb = L.gsr_interpolate_cut_backward_act(*head, ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), 0, *[ptr(t) for t in g],
                                            *[ptr(t) for t in grads], st)
    torch.cuda.synchronize()
    return rf, rb, [o.cpu().numpy() for o in outs], [x.cpu().numpy() for x in grads]


ZERO_CASES = {
    "tail0": (300, 0, [5, 7, 299, 0], (3, 4, 48, 1, 3)),
    "no_rows": (300, 17, None, (3, 4, 48, 1, 3)),
    "empty_rows": (300, 17, [], (3, 1)),
    "nothing": (300, 0, None, (3, 4)),
    "tail_N": (257, 257, [3], (3, 4, 48)),
    "N1_row": (1, 0, [0], (3, 48)),
    "N1_tail": (1, 1, None, (1, 4)),
    "eight_arrays": (1025, 65, list(range(0, 1025, 7)), (1, 2, 3, 4, 7, 16, 47, 48)),
    "out_of_range_and_duplicates": (513, 3, [-1, 513, 518, -513, 2 ** 40, -2 ** 40, 4, 4, 4, 512, 0, 255, 256, 255], (3, 4, 48, 1)),
    "more_rows_than_N": (64, 1, [k % 70 - 3 for k in range(700)], (5, 9)),
}


@pytest.mark.parametrize("name", list(ZERO_CASES))
def test_zero_grad_rows(name):
    """Against indexing, exactly; a listed row outside [0, N) is skipped."""
    from gs_train.post import zero_grad_rows
    N, tail, rows, widths = ZERO_CASES[name]
    g = torch.Generator(device=DEV).manual_seed(N + tail)
    ts = [torch.randn(N, w_, generator=g, device=DEV) + 3 for w_ in widths]
    want = [t.clone() for t in ts]
    valid = [r for r in rows or [] if 0 <= r < N]
    for t in want:
        if tail:
            t[N - tail:] = 0
        if valid:
            t[torch.tensor(valid, device=DEV)] = 0
    zero_grad_rows(ts, tail, None if rows is None else torch.tensor(rows, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    for a, b in zip(ts, want):
        assert torch.equal(a, b)
    locked = tail + len(set(valid) - set(range(N - tail, N)))
    assert all(int((b == 0).all(1).sum()) == locked for b in want)


def test_zero_grad_rows_refuses_nine_arrays():
    from gs_train.post import zero_grad_rows
    ts = [torch.ones(10, 2, device=DEV) for _ in range(9)]
    with pytest.raises(RuntimeError, match="at most 8"):
        zero_grad_rows(ts, 2, None)
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for t in ts)


def _weights_hip(idx, target, nodes, boxes, v, room=3):
    from gaussian_hierarchy._C import get_interpolation_weights
    n = len(idx)
    w = torch.full((n + room,), -7.0, device=DEV)
    k = torch.full((n + room,), -7, dtype=torch.int32, device=DEV)
    get_interpolation_weights(_dev(idx, torch.int32), float(target), _dev(nodes), _dev(boxes), torch.tensor(v),
                              torch.zeros(3), w, k)
    torch.cuda.synchronize()
    assert bool((w[n:] == -7).all()) and bool((k[n:] == -7).all())
    return w[:n].cpu().numpy(), k[:n].cpu().numpy()


def test_interpolation_weights_on_the_rule_s_boundaries():
    """get_interpolation_weights on hand-built hierarchies of 3 to 300 nodes whose every decision sits
    on or one float32 step off its bound, against the float64 rule (exact by construction:
    tests/test_cut_cases_cpu.py) and the C restatement, exactly."""
    import gs_oracle as O
    for name, nodes, boxes, v, target in C.weight_queries():
        idx = np.arange(len(nodes), dtype=np.int32)[::-1].copy()
        w, k = _weights_hip(idx, target, nodes, boxes, v)
        rw, rk, exact = R.interpolation_weights(idx, target, nodes, boxes, v)
        assert exact.all()
        ow, ok = O.interpolation_weights(idx, np.float32(target), nodes, boxes, np.asarray(v, np.float32))
        assert np.array_equal(w.astype(np.float64), rw) and np.array_equal(k, rk), name
        assert np.array_equal(w, ow) and np.array_equal(k, ok), name
    nodes, boxes = C.same_distance_hierarchy(299)
    order = np.random.default_rng(0).permutation(300).astype(np.int32)
    for n in (1, 255, 256, 257):
        for target in (0.75, 0.625):
            w, k = _weights_hip(order[:n], target, nodes, boxes, (5.0, 0.0, 0.0))
            rw, rk, _ = R.interpolation_weights(order[:n], target, nodes, boxes, (5.0, 0.0, 0.0))
            assert np.array_equal(w.astype(np.float64), rw) and np.array_equal(k, rk), (n, target)
