"""GPU parity under posed cameras and at the rasterizer's clamps (tests/posed_cases.py).

Every other parity file renders through the identity camera at the origin, where the view rotation,
the translation row, campos and the off-diagonal projection entries are ones and zeros, and its
scenes never reach the 1.3 * tanfov clamp of the view-space mean, the 0.99 alpha cap or (beyond a
handful of channels) the SH colour clamp.  Here the same pipeline -- make_scene, run_oracle, run_hip
and compare of test_gpu_parity.py, with its bars -- runs under the reference's own camera 1
(golden/cameras.npz), a steep pose (yaw 140, pitch -35, roll 70 degrees, t = (3, -7.5, 11)) and
with those three populations present; the oracle is vouched for on such inputs against fp64 autograd
in test_oracle.py.  The gradient bar (GRAD_TOL, relative L2) is applied to each whole tensor and
again to the rows of each claimed population alone: a few hundred wrong rows among thousands of
right ones would pass the first.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import posed_cases as PC
from helpers import deterministic, psnr, settings, torch_inputs
from test_gpu_parity import (binning_mode, compare, precomputed_inputs, run_hip, run_oracle, upstream_grads)

pytestmark = pytest.mark.gpu

STEEP_ALL = dict(name="posed_steep_all", pose="steep", P=1500, W=70, H=50, deg=2, seed=43, log_scale=-2.0,
                 primx=0.35, primy=0.6, edge=0.3, opaque=0.3, dark=2.0)
CASES = [
    dict(name="posed_cam1_deg3", pose="cam1", P=1500, W=96, H=64, deg=3, seed=61, log_scale=-3.0),
    dict(name="posed_steep_deg3", pose="steep", P=2000, W=96, H=64, deg=3, seed=62, log_scale=-3.0),
    STEEP_ALL,
    dict(name="posed_steep_modifier_nodepth", pose="steep", P=1500, W=96, H=64, deg=3, seed=64, log_scale=-3.0,
         scale_modifier=1.7, do_depth=False),
    dict(name="posed_steep_coarse_M4", pose="steep", P=1500, W=96, H=64, deg=1, seed=65, log_scale=-3.0, M=4),
    # footprints over tens of superblocks, centred off screen (the binning's wave-wide path); half
    # of the 300 rows moved so that 100 of them carry a position gradient
    dict(name="posed_steep_big_sb", pose="steep", P=300, W=640, H=480, deg=1, seed=49, log_scale=-0.5, edge=0.5),
    # the clamp populations alone, under the identity camera: separates them from the pose
    dict(name="identity_all", pose="identity", P=1500, W=96, H=64, deg=3, seed=47, log_scale=-2.0, edge=0.3,
         opaque=0.2, dark=2.0),
]
BY_NAME = {c["name"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's scene, upstream gradients, oracle state and gradients and row subsets: computed
    once, shared by the tests (nothing writes to them)."""
    c = BY_NAME[name]
    s = PC.make_scene(c)
    dcol, dinv = upstream_grads(c)
    st, g = run_oracle(s, c, dcol, dinv)
    masks = PC.subsets(s, st)
    PC.assert_populated(masks, g, PC.claims(c))
    if c.get("pose", "identity") != "identity":
        assert not np.array_equal(s["view"].reshape(4, 4)[:3, :3], np.eye(3, dtype=np.float32))
    assert int((st["radii"] > 0).sum()) >= 0.8 * c["P"]
    return s, dcol, dinv, st, g, {k: masks[k] for k in PC.claimed_subsets(c)}


@pytest.mark.parametrize("mode", [0, 1], ids=["local_sort", "global_sort"])
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_posed_parity_vs_oracle(name, mode):
    """test_parity_vs_oracle's comparison (bit-exact binning, image, inverse depth, gradients: its
    bars) under posed cameras and with the clamp populations, plus GRAD_TOL over each claimed
    population's rows alone and the SH clamp flags bit for bit."""
    c = BY_NAME[name]
    s, dcol, dinv, st, g, sub = reference(name)
    with binning_mode(mode):
        h = run_hip(s, c, dcol, dinv)
    compare(dict(c, name=f"{name}_{'global' if mode else 'local'}"), st, g, h, global_sort=mode == 1, subsets=sub)


def test_posed_precomputed_paths():
    """test_precomputed_paths_and_cross_identity's checks on posed_steep_all: colors_precomp /
    cov3D_precomp against the oracle (rows past the 1.3 * tanfov clamp and capped alphas included,
    each also on their own), and the cross-path identity with the (shs, scales, rotations) frame."""
    c = STEEP_ALL
    s, dcol, dinv, _, _, _ = reference(c["name"])
    colors, cov = precomputed_inputs(s, c["deg"])
    st, g = run_oracle(s, c, dcol, dinv, colors_precomp=colors, cov3D_precomp=cov)
    masks = PC.subsets(s, st)
    PC.assert_populated(masks, g, ("edge", "opaque"))
    h = run_hip(s, c, dcol, dinv, colors_precomp=colors, cov3D_precomp=cov)
    compare(dict(c, name="posed_precomp"), st, g, h, subsets={k: masks[k] for k in ("beyond", "capped")})
    base = run_hip(s, c, dcol, dinv)
    assert psnr(base["color"], h["color"]) > 60.0
    assert float(np.mean(base["radii"] != h["radii"])) < 1e-2


def test_camera_tensors_as_the_reference_builds_them():
    """scene/cameras.py:96-98 hands the rasterizer transposed views of row-major matrices
    (world_view_transform = W2C.transpose(0, 1), not contiguous).  Such tensors give the bits the
    contiguous ones give: image, inverse depth, radii, every gradient (deterministic backward) and
    mark_visible, through the function and through the module method."""
    import torch
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    c = BY_NAME["posed_steep_deg3"]
    s, dcol, dinv, st, _, _ = reference(c["name"])
    dev = torch.device("cuda:0")
    rs = settings(s, dev, c["deg"])
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    view_t = t(s["view"].reshape(4, 4).T).transpose(0, 1)
    proj_t = t(s["proj"].reshape(4, 4).T).transpose(0, 1)
    assert not view_t.is_contiguous() and not proj_t.is_contiguous()
    assert torch.equal(view_t, rs.viewmatrix) and torch.equal(proj_t, rs.projmatrix)
    outs = []
    with deterministic():
        for r in (rs, rs._replace(viewmatrix=view_t, projmatrix=proj_t)):
            inp = torch_inputs(s, dev)
            color, radii, invd = GaussianRasterizer(r)(**inp)
            ((color * torch.tensor(dcol, device=dev)).sum() + (invd * torch.tensor(dinv, device=dev)).sum()).backward()
            vis = _C.mark_visible(inp["means3D"].detach(), r.viewmatrix, r.projmatrix)
            vis2 = GaussianRasterizer(r).markVisible(inp["means3D"].detach())
            outs.append(dict(color=color.detach(), invd=invd.detach(), radii=radii, vis=vis, vis2=vis2,
                             **{"grad_" + k: v.grad for k, v in inp.items()}))
    a, b = outs
    np.testing.assert_array_equal(a["radii"].cpu().numpy(), st["radii"])
    assert 0 < int(a["vis"].sum()) and torch.equal(a["vis"], a["vis2"])
    assert float(a["grad_means3D"].abs().sum()) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k
