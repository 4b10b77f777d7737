"""GPU tests of the native post-optimisation iteration and the stage around it
(gs_train.native_post.NativePostStep, gs_train.post_stage) on the problem of
test_gpu_post.test_post_step_matches_reference_formulation: 60 000 leaves, 320 x 240, 3 views,
2000 skybox rows, 500 anchors, the limits 0.004 / 0.02 / 0.05 through limit_fn.

Which bar holds NativePostStep to PostTrainStep is decided by the run itself: PostTrainStep is run
twice from one start under helpers.deterministic(); if the two agree bit for bit (the blend's parent
accumulation uses float atomics, so this is not known beforehand) the native step must equal it bit
for bit -- parameters, moments, losses -- after 1 and 3 steps, otherwise it must be within
assert_adam_trajectories_close with test_gpu_post's atol rule and learning rates.  The branch taken
and the margins go to record_margins (profiles/r27_post_margins.jsonl).
"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("xyz", "features", "opacity", "scaling", "rotation")
ATTRS = ("_xyz", "_features", "_opacity", "_scaling", "_rotation")
LIMITS = [0.004, 0.02, 0.05]


_BASES = {}


def _base(leaves=60_000, W=320, H=240, skybox=2000, anchors=500):
    """The problem, built once per size: synthetic_lod_hierarchy orders its leaves with an unstable
    argsort, so two builds from one seed may differ in row order; every step under comparison runs on
    a clone of ONE build's model, with its targets, masks and exposures."""
    from gs_train.post import PostTrainStep, synthetic_post_problem
    key = (leaves, W, H, skybox, anchors)
    if key not in _BASES:
        torch.manual_seed(0)
        _BASES[key] = synthetic_post_problem(leaves, W, H, n_views=3, skybox=skybox, n_anchors=anchors, seed=2,
                                             step_cls=PostTrainStep)
    return _BASES[key]


def _problem(step_cls, fixed_limits=True, options=None, **kw):
    """A step of step_cls on a clone of the base problem's model (options: other constructor options
    than the base's alpha masks and exposures)."""
    from gs_train.post import HierarchyModel
    from gs_train.synthetic import orbit_cameras
    base = _base(**kw)
    m = base.m
    c = lambda t: t.detach().clone()
    model = HierarchyModel(c(m._xyz), c(m._features), c(m._opacity), torch.exp(c(m._scaling)), c(m._rotation), m.nodes,
                           m.boxes, skybox=m.skybox_points, anchors=m.anchors, device=DEV)
    opts = dict(alpha_masks=base.amask, exposures=base.expo) if options is None else options
    post = step_cls(model, orbit_cameras(3, base.W, base.H), base.gts, base.W, base.H, **opts)
    if fixed_limits:
        post.limit_fn = lambda it: LIMITS[(it - 1) % 3]
    return post


def _snap(post):
    m = post.m
    out = {n: getattr(m, a).detach().clone() for n, a in zip(NAMES, ATTRS)}
    for n, a in zip(NAMES, ATTRS):
        st = post.optimizer.state.get(getattr(m, a), {})
        if "exp_avg" in st:
            out["m_" + n], out["v_" + n] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _lrs(post, steps):
    from gs_train.post import POST_LR
    col_lr = torch.full((1, post.m._features.shape[1], 1), POST_LR["feature_lr"] / 20.0, device=DEV)
    col_lr[:, 0] = POST_LR["feature_lr"]
    return dict(xyz=max(post.xyz_lr(it) for it in range(0, steps + 2)), features=col_lr,
                opacity=POST_LR["opacity_lr"], scaling=POST_LR["scaling_lr"], rotation=POST_LR["rotation_lr"])


def _assert_close(tag, post, got, want, init, steps):
    """test_gpu_post's bar: the Adam travel bound per element, the bulk within atol."""
    from helpers import assert_adam_trajectories_close, record_margins
    lrs = _lrs(post, steps)
    for name in NAMES:
        atol = 2e-6 + 1e-3 * (got[name] - init[name]).abs().max().item()
        worst, close = assert_adam_trajectories_close(name, got[name], want[name], init[name], lrs[name], steps, atol)
        record_margins(f"{tag}_step{steps}_{name}", travel_frac=worst, close=close)


def _run(step_cls, steps=3, **kw):
    """Snapshots after steps 1 and 3 and the losses; for a native step also what each step left."""
    post = _problem(step_cls, **kw)
    init = _snap(post)
    snaps, losses, extra = {}, [], []
    for i in range(1, steps + 1):
        losses.append(post.step().item())
        if hasattr(post, "grads"):
            live, stamp, cur = post.row_state()
            extra.append(dict(grads_zero=all(int((_bits(g) != 0).sum()) == 0 for g in post.grads.values()),
                              live=live, stamp=stamp, cur=cur, cut=post.last_cut, growths=post.ctx_stats()["growths"]))
        if i in (1, 3):
            snaps[i] = _snap(post)
    return dict(post=post, init=init, snaps=snaps, losses=losses, extra=extra)


@pytest.fixture(scope="module")
def runs():
    from gs_train.native_post import NativePostStep
    from gs_train.post import PostTrainStep
    from helpers import deterministic, record_margins
    with deterministic():
        a, b, n = _run(PostTrainStep), _run(PostTrainStep), _run(NativePostStep)
    bitwise = a["losses"] == b["losses"] and all(_same_bits(a["snaps"][i], b["snaps"][i]) for i in (1, 3))
    record_margins("post_native_branch", python_runs_agree_bitwise=float(bitwise))
    print(f"\nPostTrainStep twice from one start: {'bitwise equal' if bitwise else 'NOT bitwise equal'}")
    return dict(python=a, python2=b, native=n, bitwise=bitwise)


def _hold(tag, runs, native, python, steps_list=(1, 3)):
    """The bar chosen by the run: bits, or the Adam trajectory bar."""
    from helpers import record_margins
    if runs["bitwise"]:
        assert native["losses"] == python["losses"], tag
        for i in steps_list:
            for k in python["snaps"][i]:
                a, b = native["snaps"][i][k], python["snaps"][i][k]
                assert torch.equal(_bits(a), _bits(b)), (tag, i, k, int((_bits(a) != _bits(b)).sum()))
        record_margins(f"{tag}_bitwise", equal=1.0)
    else:
        np.testing.assert_allclose(native["losses"], python["losses"], rtol=2e-5, atol=1e-7)
        for i in steps_list:
            _assert_close(tag, native["post"], native["snaps"][i], python["snaps"][i], native["init"], i)


def test_native_step_equals_python_step(runs):
    assert all(c > 1000 for c in (e["cut"] for e in runs["native"]["extra"]))
    assert _same_bits(runs["native"]["init"], runs["python"]["init"])
    _hold("post_native_vs_python", runs, runs["native"], runs["python"])
    # the moments are the optimizer's own state tensors, .grad stays None
    post = runs["native"]["post"]
    assert all(getattr(post.m, a).grad is None for a in ATTRS)
    assert "m_xyz" in runs["native"]["snaps"][3]
    assert [post.optimizer.state[getattr(post.m, a)]["step"].item() for a in ATTRS] == [3.0] * 5


def test_native_step_matches_reference_formulation():
    """NativePostStep held to ReferencePostStep by test_gpu_post's bars, unchanged (the default atomic
    backward, as there)."""
    from gs_train.native_post import NativePostStep
    from train_torch_ref import ReferencePostStep
    post = _problem(NativePostStep)
    ref = ReferencePostStep(post)
    m = post.m
    init = _snap(post)
    la, lb = [], []
    for i in range(3):
        la.append(post.step().item())
        lb.append(ref.step(i % 3, LIMITS[i % 3]).item())
        assert post.last_cut > 1000
        if i in (0, 2):
            steps = i + 1
            np.testing.assert_allclose(la, lb, rtol=2e-5, atol=1e-7)
            want = dict(zip(NAMES, (ref._xyz.detach(), ref.features().detach(), ref._opacity.detach(),
                                    ref._scaling.detach(), ref._rotation.detach())))
            _assert_close("post_native_vs_reference", post, _snap(post), want, init, steps)
    S = m.skybox_points
    for n, a in zip(NAMES, ATTRS):
        x = getattr(m, a).detach()
        assert torch.equal(x[-S:], init[n][-S:]) and torch.equal(x[m.anchors], init[n][m.anchors])


def test_gradients_zero_and_locked_rows_fixed(runs):
    n = runs["native"]
    assert [e["grads_zero"] for e in n["extra"]] == [True, True, True]
    m = n["post"].m
    S = m.skybox_points
    for i in (1, 3):
        for name in NAMES:
            x, x0 = n["snaps"][i][name], n["init"][name]
            assert torch.equal(_bits(x[-S:]), _bits(x0[-S:])), name
            assert torch.equal(_bits(x[m.anchors]), _bits(x0[m.anchors])), name
            assert not torch.equal(x, x0), name


def test_never_stamped_rows_keep_bits_and_idle_live_rows_exist(runs):
    n = runs["native"]
    last = n["extra"][-1]
    never = last["stamp"] == 0
    idle_live = (last["live"] != 0) & (last["stamp"] != last["cur"])
    print(f"\nrows {never.numel()}: never stamped {int(never.sum())}, idle live at step 3 {int(idle_live.sum())}, "
          f"live {int((last['live'] != 0).sum())}, cuts {[e['cut'] for e in n['extra']]}")
    # both paths of the kernel are exercised on this problem over the three limits
    assert int(never.sum()) > 0 and int(idle_live.sum()) > 0
    for name in NAMES:
        assert torch.equal(_bits(n["snaps"][3][name][never]), _bits(n["init"][name][never])), name
        assert int((_bits(n["snaps"][3]["m_" + name][never]) != 0).sum()) == 0, name
        assert int((_bits(n["snaps"][3]["v_" + name][never]) != 0).sum()) == 0, name
    assert int(last["live"][never].sum()) == 0
    # an idle live row kept moving at step 3 on its decaying moments, as under the dense Adam
    p = runs["python"]
    moved = (p["snaps"][3]["xyz"] != p["snaps"][1]["xyz"]).any(1)
    assert bool((moved & idle_live).any())


def test_context_growth_stops_after_the_largest_cut(runs):
    post = runs["native"]["post"]  # three more steps: the limits cycle, nothing is larger than before
    before = post.ctx_stats()
    for _ in range(3):
        post.step()
    after = post.ctx_stats()
    assert after["growths"] == before["growths"] and after["bytes"] == before["bytes"] and after["stream_ordered"]
    assert runs["native"]["extra"][0]["growths"] > 0


SMALL = dict(leaves=20_000, W=192, H=144, skybox=500, anchors=100)


def _pair(runs, tag, **kw):
    from gs_train.native_post import NativePostStep
    from gs_train.post import PostTrainStep
    from helpers import deterministic
    with deterministic():
        p, n = _run(PostTrainStep, **kw), _run(NativePostStep, **kw)
    _hold(tag, runs, n, p)
    assert all(e["grads_zero"] for e in n["extra"])
    return p, n


def test_no_skybox_no_anchors_root_parent_stamps_last_row(runs):
    """S = 0 and no anchors: a root's parent -1 names the last ordinary row (weight 0), which is then
    stamped and updated like any other."""
    from gs_train.native_post import NativePostStep
    from gs_train.post import PostTrainStep
    kw = dict(SMALL, skybox=0, anchors=0)
    p, n = _pair(runs, "post_native_s0", **kw)
    post = p["post"]
    N = post.m.N
    assert post.m.skybox_points == 0 and post.m.anchors.numel() == 0
    # a limit so coarse that the cut is the roots alone: row N - 1 (a leaf) is no child of this cut,
    # so only the wrap of the parent -1 can stamp it
    coarse = 1e6
    cut = post.cut(0, coarse)
    assert cut >= 1 and bool((post.pi[:cut] < 0).all()) and not bool((post.ri[:cut] == N - 1).any())
    nat, py = _problem(NativePostStep, **kw), _problem(PostTrainStep, **kw)
    nat.limit_fn = py.limit_fn = lambda it: coarse
    x0 = nat.m._xyz.detach().clone()
    la, lb = nat.step().item(), py.step().item()
    live, stamp, cur = nat.row_state()
    assert nat.last_cut == cut and cur == 1 and int(stamp[N - 1]) == cur and int(live[N - 1]) == 1
    assert int((stamp == cur).sum()) == cut + 1
    np.testing.assert_allclose(la, lb, rtol=2e-5, atol=1e-7)
    # the wrapped row's gradient has weight 1 - t = 0: it is stamped, cleared and does not move
    assert torch.equal(nat.m._xyz.detach()[N - 1], x0[N - 1]) and torch.equal(py.m._xyz.detach()[N - 1], x0[N - 1])
    assert all(int((_bits(g) != 0).sum()) == 0 for g in nat.grads.values())


def test_odd_image_size(runs):
    _pair(runs, "post_native_251x189", **dict(SMALL, W=251, H=189))


def test_no_exposure_no_alpha_mask_clamps_only(runs):
    from gs_train.native_post import NativePostStep
    from gs_train.post import PostTrainStep
    from helpers import deterministic
    with deterministic():
        p, n = (_run(cls, options=dict(alpha_masks=None, exposures=None), **SMALL) for cls in (PostTrainStep, NativePostStep))
    assert all(e is None for e in n["post"].expo + n["post"].amask)
    _hold("post_native_clamp_only", runs, n, p)


def test_checkpoint_continues_bit_for_bit(runs):
    """capture at iteration 2 of a 4-iteration TrainPost.run, restored into a fresh step, gives the
    uninterrupted run's bits at iteration 4 -- the random limit draws included (no limit_fn)."""
    from gs_train.native_post import NativePostStep
    from gs_train.post import PostTrainStep
    from gs_train.post_stage import TrainPost, restore
    from helpers import deterministic
    with deterministic():
        finals, caps, inits = {}, {}, {}
        for cls in (NativePostStep, PostTrainStep):
            step = _problem(cls, fixed_limits=False, **SMALL)
            inits[cls] = _snap(step)
            torch.manual_seed(5)
            grabbed = {}
            TrainPost(step, checkpoint_iterations=(2,), on_checkpoint=lambda it, c: grabbed.update(c)).run(until=4)
            assert step.iteration == 5 and int(grabbed["iteration"]) == 3
            finals[cls], caps[cls] = _snap(step), grabbed
        # native capture -> fresh native step: the set-up is redone on the replaced tensors
        fresh = _problem(NativePostStep, fixed_limits=False, **SMALL)
        fresh.step()  # a set-up on its own tensors first, then the restore replaces them
        grads_before = fresh.grads
        torch.manual_seed(99)  # the restore brings the generator's state back
        restore(fresh, caps[NativePostStep])
        TrainPost(fresh).run(until=4)
        assert fresh.grads is not grads_before  # set-up redone
        assert _same_bits(_snap(fresh), finals[NativePostStep])
        # python capture -> python step: bit for bit if the python step is reproducible at all
        again = _problem(PostTrainStep, fixed_limits=False, **SMALL)
        restore(again, caps[PostTrainStep])
        TrainPost(again).run(until=4)
        if runs["bitwise"]:
            assert _same_bits(_snap(again), finals[PostTrainStep])
        # python capture -> native step, within the bar the run chose
        cross = _problem(NativePostStep, fixed_limits=False, **SMALL)
        restore(cross, caps[PostTrainStep])
        TrainPost(cross).run(until=4)
        got, want = _snap(cross), finals[PostTrainStep]
        if runs["bitwise"]:
            assert _same_bits(got, want)
        else:
            _assert_close("post_native_cross_restore", cross, got, want, inits[PostTrainStep], 4)


def test_stage_round_trip(tmp_path):
    """build_hierarchy -> .save -> load_hierarchy_model (+ a scaffold's skybox rows, anchors.bin) ->
    three native iterations -> save_hier -> hier_merge.load_chunk: the file's rows are the model's."""
    from gs_train.hier_build import build_hierarchy
    from gs_train.hier_merge import load_chunk
    from gs_train.native_post import NativePostStep
    from gs_train.post_stage import TrainPost, load_hierarchy_model, save_hier
    from gs_train.scaffold import save_scaffold
    from gs_train.synthetic import camera, orbit_cameras
    import types
    W, H, P, S = 192, 144, 5000, 300
    g = torch.Generator(device=DEV).manual_seed(7)
    u = lambda *s: torch.rand(*s, generator=g, device=DEV)
    _, _, _, tx, ty = camera(W, H)
    z = 2 + 18 * u(P)
    xyz = torch.stack([(u(P) * 1.9 - 0.95) * tx * z, (u(P) * 1.9 - 0.95) * ty * z, z], 1)
    shs = 0.05 * torch.randn(P, 16, 3, generator=g, device=DEV)
    shs[:, 0] = 0.5 * torch.randn(P, 3, generator=g, device=DEV)
    hier = build_hierarchy(xyz, -3.5 + 0.3 * torch.randn(P, 3, generator=g, device=DEV),
                           torch.randn(P, 4, generator=g, device=DEV), 0.05 + 0.9 * u(P, 1), shs)
    path = str(tmp_path / "chunk.hier")
    hier.save(path)
    N = hier.nodes.shape[0]
    d = torch.randn(400, 3, generator=g, device=DEV)
    d[:, 2] = d[:, 2].abs() + 0.5
    sky = types.SimpleNamespace(_xyz=60 * d / d.norm(dim=1, keepdim=True), _opacity=torch.randn(400, 1, generator=g, device=DEV),
                                _scaling=torch.full((400, 3), 0.5, device=DEV), _rotation=torch.randn(400, 4, generator=g, device=DEV),
                                get_features=0.3 * torch.randn(400, 4, 3, generator=g, device=DEV))
    save_scaffold(str(tmp_path / "scaffold"), sky, S)
    anchors = np.arange(10, 500, 7, dtype="<i4")
    with open(str(tmp_path / "anchors.bin"), "wb") as f:
        f.write(np.asarray([len(anchors)], "<u4").tobytes() + anchors.tobytes())
    model, expos = load_hierarchy_model(path, str(tmp_path / "scaffold"), device=DEV)
    assert expos is None and model.N == N + S and model.skybox_points == S and model.anchors.numel() == len(anchors)
    cams = orbit_cameras(3, W, H)
    tmp = NativePostStep(model, cams, [None] * 3, W, H)
    gts = []
    with torch.no_grad():
        for k in range(3):
            gts.append(tmp.render(k, tmp.cut(k, 0.05))[0].contiguous())
    del tmp
    step = NativePostStep(model, cams, gts, W, H)
    step.limit_fn = lambda it: 0.01
    before = model._xyz.detach().clone()
    TrainPost(step).run(until=3)
    assert step.iteration == 4 and not torch.equal(before[:N], model._xyz.detach()[:N])
    assert torch.equal(before[N:], model._xyz.detach()[N:])
    out = path + "_opt"
    save_hier(model, out)
    back = load_chunk(out, DEV)
    for got, want in ((back.means3D, model._xyz), (back.log_scales, model._scaling), (back.rotations, model._rotation),
                      (back.opacities, model._opacity.abs()), (back.shs, model._features)):
        assert torch.equal(got, want.detach()[:N])
    assert torch.equal(back.nodes, model.nodes) and os.path.getsize(out) > os.path.getsize(path)


def test_synthetic_post_problem_builds_a_native_step():
    from gs_train.native_post import NativePostStep
    from gs_train.post import synthetic_post_problem
    post = synthetic_post_problem(5000, 96, 64, n_views=2, skybox=100, n_anchors=10, seed=3, step_cls=NativePostStep)
    assert isinstance(post, NativePostStep)
    losses = [post.step().item() for _ in range(2)]
    assert all(np.isfinite(losses)) and post.last_cut > 0 and post.iteration == 3
