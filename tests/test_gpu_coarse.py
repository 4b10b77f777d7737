"""GPU tests of the coarse scaffold stage (gs_train.coarse): CoarseTrainStep against
train_coarse.py:94-145 in the reference's formulation (tests/coarse_ref.py), and the stage end to
end: cloud -> model -> TrainCoarse -> scaffold files -> a chunk's model -> train steps, hierarchy."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
P, SKY = 3000, 64
NAMES = ("_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def _problem(fused, size, alpha, **kw):
    from coarse_ref import reference_coarse_step_cls
    from gs_train.coarse import CoarseTrainStep
    from gs_train.harness import make_problem
    torch.manual_seed(0)
    cls = CoarseTrainStep if fused else reference_coarse_step_cls()
    ts = make_problem(P, *size, n_views=4, seed=1, sh_degree=1, step_cls=cls, depth=False, alpha=alpha,
                      skybox_points=SKY, **kw)
    with torch.no_grad():
        ts.g._xyz[0] = torch.tensor([0.0, 0.0, -500.0], device=DEV)  # row 0 behind every camera: never relevant
    return ts


def _state(ts, name):
    return ts.optimizer.state[getattr(ts.g, name)]


def _snapshot(ts):
    return {n: getattr(ts.g, n).detach().clone() for n in NAMES + ("_xyz",)}


@pytest.mark.parametrize("size,alpha", [((96, 64), False), ((96, 64), True), ((101, 67), True), ((101, 67), False)])
def test_coarse_step_matches_reference_structured_step(size, alpha):
    """Three iterations of the fused coarse step against the reference-structured one: the losses
    and every parameter's Adam trajectory within the bars of
    test_train_step_fused_matches_reference_structured_step (rtol 1e-5 / atol 1e-6 on the loss,
    helpers.assert_adam_trajectories_close with atol 1e-5), at M = 4 with 64 skybox rows; 101 x 67 is
    ragged for the SSIM strips and the tiles.  After the first iteration row 0 -- invisible, so never
    relevant itself -- is given nonzero opacity moments on both sides: the (R, 2) index updates it."""
    from gs_train.harness import LR
    from helpers import assert_adam_trajectories_close, record_margins
    runs = {}
    for fused in (True, False):
        ts = _problem(fused, size, alpha)
        assert ts.g.get_features.shape == (P, 4, 3)
        init = _snapshot(ts)
        losses = [ts.step().item()]
        for key, v in (("exp_avg", 1e-3), ("exp_avg_sq", 1e-6)):
            _state(ts, "_opacity")[key][0] = v
        after1 = _snapshot(ts)
        losses += [ts.step().item() for _ in range(2)]
        m_xyz = _state(ts, "_xyz")["exp_avg"].clone()
        if not fused:
            assert ts.last_relevant.dim() == 2 and ts.last_relevant.shape[1] == 2  # the quirk's index
            assert 0 < ts.last_relevant.shape[0] < P and not bool((ts.last_relevant[:, 0] == 0).any())
        runs[fused] = (losses, _snapshot(ts), init, after1, m_xyz, ts)
    (la, pa, ia, a1, ma, ta), (lb, pb, _, b1, mb, _) = runs[True], runs[False]
    np.testing.assert_allclose(la, lb, rtol=1e-5, atol=1e-6)
    lrs = dict(_features_dc=LR["feature_lr"], _features_rest=LR["feature_lr"] / 20.0, _opacity=LR["opacity_lr"],
               _scaling=LR["scaling_lr"], _rotation=LR["rotation_lr"])
    for n in NAMES:
        worst, close = assert_adam_trajectories_close(n, pa[n], pb[n], ia[n], lrs[n], 3, atol=1e-5)
        record_margins(f"coarse_step_{size[0]}x{size[1]}_{alpha}{n}", travel_frac=worst, close=close)
    # xyz never changes (rate 0) while its moments advance
    assert torch.equal(pa["_xyz"], ia["_xyz"]) and torch.equal(pb["_xyz"], ia["_xyz"])
    assert bool((ma != 0).any())
    assert torch.isclose(ma, mb, rtol=1e-3, atol=1e-9).float().mean().item() >= 0.999
    # row 0: not relevant (zero gradient), yet its opacity moved in iterations 2 and 3, as the reference's
    assert pa["_opacity"][0] != a1["_opacity"][0] and pb["_opacity"][0] != b1["_opacity"][0]
    assert torch.equal(a1["_opacity"][0], ia["_opacity"][0])
    assert abs(float(pa["_opacity"][0] - pb["_opacity"][0])) <= 1e-5
    # the skybox rows train, their scaling aside
    sky = slice(1, SKY)
    assert bool((pa["_opacity"][sky] != ia["_opacity"][sky]).any())
    assert bool((pa["_features_dc"][sky] != ia["_features_dc"][sky]).any())
    assert torch.equal(pa["_scaling"][:SKY], ia["_scaling"][:SKY])
    # the statistics: max_radii2D only
    g = ta.g
    assert not g.xyz_gradient_accum.any() and not g.denom.any() and bool((g.max_radii2D > 0).any())
    # the same rasterizer on parameters a few ulps apart: the radii agree but for a rare rounding of one
    assert (g.max_radii2D == runs[False][5].g.max_radii2D).float().mean().item() >= 0.999
    assert g._exposure.grad is None


def test_coarse_step_dense_fallback_when_no_row_is_relevant():
    """All opacities driven to about 0 (logit -30): nothing is blended, every opacity gradient is
    zero, and Adam.step gets an empty index: the dense update.  With moments planted in every
    row's rotation, every row moves -- as the reference's, within the same bars."""
    runs = {}
    for fused in (True, False):
        ts = _problem(fused, (96, 64), False)
        ts.step()
        with torch.no_grad():
            ts.g._opacity.fill_(-30.0)
        st = _state(ts, "_rotation")
        st["exp_avg"].fill_(1e-3)
        st["exp_avg_sq"].fill_(1e-6)
        before = ts.g._rotation.detach().clone()
        ts.step()
        if not fused:
            assert ts.last_relevant.numel() == 0
        runs[fused] = (before, ts.g._rotation.detach().clone())
    (b0, b1), (r0, r1) = runs[True], runs[False]
    assert bool((b1 != b0).all())  # every row, every column: the dense branch
    # the moves are ~2e-4 on unit quaternions: each side's stored value carries half an ulp of 1
    assert torch.allclose(b1 - b0, r1 - r0, rtol=1e-3, atol=5e-7)


def test_coarse_shrink_limit_and_skybox_rows():
    """The shrink's limit is 0.1 * cameras_extent (the chunk stage's is 0.02) and it starts at the
    skybox boundary: a row planted just above the limit (by 2%: an Adam step of the log-scale is at
    most about 0.5%) shrinks by 0.8, one just below it and a skybox row above it do not."""
    ts = _problem(True, (96, 64), False)
    assert ts.extent == 10.0
    above, below, sky = 200, 201, 5
    with torch.no_grad():
        ts.g._scaling[above] = math.log(1.0 * 1.02)
        ts.g._scaling[below] = math.log(1.0 * 0.98)  # five times the chunk stage's limit of 0.2
        ts.g._scaling[sky] = math.log(1.0 * 1.5)
    s0 = ts.g._scaling.detach().clone()
    ts.step()
    s1 = ts.g._scaling.detach()
    lr = 0.005  # scaling_lr: one Adam step moves an element by at most about that
    assert bool((s1[above] < s0[above] + math.log(0.8) + 2 * lr).all()) and bool((s1[above] > s0[above] + math.log(0.8) - 2 * lr).all())
    assert bool((s1[below] > s0[below] - 2 * lr).all())
    assert torch.equal(s1[sky], s0[sky])


def test_coarse_stage_end_to_end(tmp_path):
    """Cloud -> create_from_cloud(skybox_points=100, sh_degree=1) -> TrainCoarse (40 iterations,
    sh_interval 10) -> save -> load_scaffold (bit-equal) -> create_from_cloud(scaffold, bounds) ->
    three iterations of TrainStep and NativeTrainStep -> Hierarchy.to_model(skybox_rows=...)."""
    import model_init_ref as R
    from gs_train.chunk import _yaw_camera, nerfpp_radius, street_scene
    from gs_train.coarse import CoarseTrainStep, TrainCoarse
    from gs_train.harness import GaussianSet, TrainStep
    from gs_train.hier_build import build_hierarchy
    from gs_train.model_init import create_from_cloud
    from gs_train.native_step import NativeTrainStep
    from gs_train.scaffold import load_scaffold
    W, H = 128, 96
    dev = torch.device(DEV)
    torch.manual_seed(3)
    truth = street_scene(20_000, 9.0, dev, seed=0)
    cams = [_yaw_camera(W, H, (0.0, 0.0, 3.0 * k), 2 * math.pi * f / 4, 90.0) for k in range(4) for f in range(4)]
    n = len(cams)
    tg = GaussianSet(*(truth[k].cpu().numpy() for k in ("means3D", "shs", "opacities", "scales", "rotations")),
                     n_images=n, sh_degree=3, device=dev, joined_features=True)
    tmp = TrainStep(tg, cams, [None] * n, W, H)
    with torch.no_grad():
        gts = [tmp.render(k, torch.zeros(3, device=dev))[0].contiguous() for k in range(n)]
    sel = torch.randperm(20_000, device=dev)[:2000]
    pts, col = truth["means3D"][sel].contiguous(), truth["rgb"][sel].contiguous()
    extent = nerfpp_radius([c[2] for c in cams])

    g, S, K = create_from_cloud(pts, col, n_images=n, spatial_lr_scale=extent, skybox_points=100, sh_degree=1)
    assert (S, K, g.P) == (100, None, 2100) and g._features.shape == (2100, 4, 3)
    step = CoarseTrainStep(g, cams, gts, W, H, cameras_extent=extent, skybox_points=S, iterations=41)
    loop = TrainCoarse(step, iterations=41, sh_interval=10)
    losses = []
    loop.run(callback=lambda it, loss: losses.append(loss))
    assert len(losses) == 40 and step.iteration == 41 and g.active_sh_degree == 1
    losses = torch.stack(losses).cpu()
    assert bool(torch.isfinite(losses).all())
    assert float(losses[-10:].mean()) < float(losses[:10].mean())  # seeded; a direction check, not a bar

    loop.save(tmp_path / "scaffold")
    sc = load_scaffold(tmp_path / "scaffold", device=dev)
    assert sc.skybox_points == 100
    for a, b in ((sc.xyz, g._xyz), (sc.shs, g._features), (sc.opacity_raw, g._opacity), (sc.log_scales, g._scaling),
                 (sc.rotations, g._rotation)):
        assert torch.equal(a, b.detach())

    center, ext3 = [0.0, 0.0, 4.5], [6.0, 6.0, 6.0]
    g2, S2, K2 = create_from_cloud(pts, col, n_images=n, spatial_lr_scale=extent, skybox_points=100, scaffold=sc,
                                   bounds=(center, ext3), sh_degree=3)
    want = int(R.scaffold_select(sc.xyz.cpu().numpy(), 100, center, ext3).sum())
    assert S2 == 100 and K2 == want and 100 < K2 < 2100
    assert g2.P == K2 + 2000 and g2._features.shape == (g2.P, 16, 3)
    mask = torch.from_numpy(R.scaffold_select(sc.xyz.cpu().numpy(), 100, center, ext3)).to(dev)
    assert torch.equal(g2._features[:K2, :4].detach(), sc.shs[mask])
    assert not g2._features[:K2, 4:].any()
    raw = [t.detach().clone() for t in (g2._xyz, g2._features, g2._opacity, g2._scaling, g2._rotation)]
    for cls in (TrainStep, NativeTrainStep):
        from gs_train.model_init import gaussians_from_raw
        gm = gaussians_from_raw(*[t.clone() for t in raw], n_images=n, spatial_lr_scale=extent)
        ts = cls(gm, cams, gts, W, H, cameras_extent=extent, skybox_points=S2, scaffold_points=K2)
        ls = torch.stack([ts.step() for _ in range(3)]).cpu()
        assert bool(torch.isfinite(ls).all()), cls.__name__
        assert not torch.equal(gm._opacity.detach(), raw[2])

    h = build_hierarchy(g2._xyz.detach(), g2._scaling.detach(), g2._rotation.detach(), g2.get_opacity.detach(),
                        g2._features.detach(), first_row=S2)
    model = h.to_model(skybox_rows=sc.skybox_rows())
    assert model is not None
