"""Posed cameras and the rasterizer's clamp populations for the parity tests (test_oracle.py,
test_gpu_posed.py), and the row subsets on which those tests apply their bars.

The synthetic scenes (gs_oracle.synthetic_scene) are drawn in the frustum of an identity camera at
the origin: with view = I and campos = 0 a transposed view rotation, a wrong translation row, a
dropped campos in the SH direction or a projection entry read from the wrong slot are all invisible.
`pose_scene` reads such a scene's means as camera-space points and moves them to the world of a posed
camera, so the visible population stays the one the scene was drawn with.

Three branches that the plain scenes never reach are populated by `populate`:
  edge    rows whose view-space mean lies past the 1.3 * tanfov clamp (d/dtx, d/dty zeroed in the
          backward), made large enough to reach pixels;
  opaque  opacities of exactly 1.0, so that alpha = min(0.99, opacity * G) is capped;
  dark    a wide SH DC term, so that a good share of the colour channels clamps at zero.
`subsets` gives the row masks of each (from the oracle's forward state) and `assert_populated` fails
a case whose claimed population is not there: conditions on the inputs, not on the code under test.
"""
from __future__ import annotations

import math
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MIN_BEYOND, MIN_CAPPED, MIN_SHARE, COLOUR_GAP = 100, 20, 0.05, 1e-5


def _rx(a):
    return np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])


def _ry(a):
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


def _rz(a):
    return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])


def _rot(yaw, pitch, roll):
    return _rz(math.radians(roll)) @ _rx(math.radians(pitch)) @ _ry(math.radians(yaw))


def pose(name, W=None, H=None, primx=0.5, primy=0.5, nudge_deg=0.0):
    """-> dict(view, proj, campos, tanfovx, tanfovy, W, H, fovx_deg) in the rasterizer's convention.

    cam1   camera 1 of golden/cameras.npz (96x64, fov 50 deg, random rotation, T = (0.3, -0.2, 1.5),
           principal point (0.45, 0.55)): the reference's own matrices, verbatim;
    steep  yaw 140, pitch -35, roll 70 degrees, t = (3, -7.5, 11), fov 60 deg;
    mild   yaw 25, pitch 10, roll 15 degrees, t = (0.5, -0.3, 1.0): for worlds that cannot be moved.
    nudge_deg turns a steep or mild camera a little further about its own axes (a second view of a
    world posed for the first)."""
    import gs_oracle as O
    if name == "cam1":
        cams = np.load(os.path.join(GOLD, "cameras.npz"))
        k = lambda n: cams["cam1_" + n]
        assert (W is None or W == int(k("W"))) and (H is None or H == int(k("H")))
        return dict(view=k("viewmatrix").astype(np.float32), proj=k("projmatrix").astype(np.float32),
                    campos=k("campos").astype(np.float32), tanfovx=float(k("tanfovx")), tanfovy=float(k("tanfovy")),
                    W=int(k("W")), H=int(k("H")), fovx_deg=math.degrees(float(k("FoVx"))))
    if name == "steep":
        Rw2c, t = _rot(140.0, -35.0, 70.0), np.array([3.0, -7.5, 11.0])
    elif name == "mild":
        Rw2c, t = _rot(25.0, 10.0, 15.0), np.array([0.5, -0.3, 1.0])
    else:
        raise ValueError(name)
    if nudge_deg:
        N = _ry(math.radians(nudge_deg)) @ _rx(math.radians(-0.7 * nudge_deg))
        Rw2c, t = N @ Rw2c, N @ t + np.array([0.05, -0.03, 0.02]) * nudge_deg
    view, proj, campos, tx, ty = O.camera(W, H, 60.0, R=Rw2c.T, t=t, primx=primx, primy=primy)
    return dict(view=view, proj=proj, campos=campos, tanfovx=tx, tanfovy=ty, W=W, H=H, fovx_deg=60.0)


def pose_scene(s, p):
    """The scene's means3D read as camera-space points of `p` and moved to its world (float64, the
    inverse view matrix); view, proj, campos and tanfov* replaced by the pose's.  In place."""
    assert s["W"] == p["W"] and s["H"] == p["H"]
    inv = np.linalg.inv(p["view"].astype(np.float64).reshape(4, 4))
    m = s["means3D"].astype(np.float64)
    hom = np.concatenate([m, np.ones((m.shape[0], 1))], 1)
    s["means3D"] = np.ascontiguousarray((hom @ inv)[:, :3].astype(np.float32))
    s["view"], s["proj"], s["campos"] = p["view"], p["proj"], p["campos"]
    s["tanfovx"], s["tanfovy"] = p["tanfovx"], p["tanfovy"]
    return s


def populate(s, seed, edge=0.0, opaque=0.0, dark=0.0):
    """The clamp populations, on a scene still in camera space (before pose_scene).  In place."""
    P = s["means3D"].shape[0]
    if edge:
        rng = np.random.default_rng(seed + 301)
        idx = np.nonzero(rng.random(P) < edge)[0]
        n = len(idx)
        m = s["means3D"]
        z = m[idx, 2].astype(np.float64)
        which = rng.integers(0, 3, n)  # 0: x, 1: y, 2: both
        off = rng.uniform(1.3, 1.9, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
        mx, my = which != 1, which != 0
        m[idx[mx], 0] = (off[mx, 0] * s["tanfovx"] * z[mx]).astype(np.float32)
        m[idx[my], 1] = (off[my, 1] * s["tanfovy"] * z[my]).astype(np.float32)
        s["scales"][idx] = (np.exp(rng.normal(-0.3, 0.3, (n, 3))) * z[:, None] / 6.0).astype(np.float32)
    if opaque:
        rng = np.random.default_rng(seed + 302)
        o = rng.uniform(0.05, 1.0, (P, 1)).astype(np.float32)
        o[rng.random(P) < opaque] = np.float32(1.0)
        s["opacities"] = o
    if dark:
        rng = np.random.default_rng(seed + 303)
        s["shs"][:, 0, :] = rng.normal(0, dark, (P, 3)).astype(np.float32)
    return s


def make_scene(c):
    """A case dict of test_gpu_parity.make_scene plus pose = identity | cam1 | steep | mild and the
    populations edge / opaque / dark."""
    from test_gpu_parity import make_scene as base_scene
    name = c.get("pose", "identity")
    p = None
    if name != "identity":
        p = pose(name, c["W"], c["H"], c.get("primx", 0.5), c.get("primy", 0.5))
        c = dict(c, fovx=p["fovx_deg"])
    s = base_scene(c)
    populate(s, c["seed"], c.get("edge", 0.0), c.get("opaque", 0.0), c.get("dark", 0.0))
    return pose_scene(s, p) if p is not None else s


def steep_world(P, W, H, seed, n_views=2, nudge_deg=3.0):
    """(scene, cameras) for gs_train.harness.make_problem(world=...): the seeded training scene
    moved to the steep pose's world, seen by that camera and by ones turned nudge_deg further each."""
    from gs_train.synthetic import synthetic_scene
    s = pose_scene(synthetic_scene(P, W, H, seed=seed, sh_degree=3), pose("steep", W, H))
    cams = []
    for k in range(n_views):
        p = pose("steep", W, H, nudge_deg=k * nudge_deg)
        cams.append((p["view"], p["proj"], p["campos"], p["tanfovx"], p["tanfovy"]))
    return s, cams


def claims(c):
    return tuple(k for k in ("edge", "opaque", "dark") if c.get(k))


def claimed_subsets(c):
    """The subsets a case's bars apply to: those of the populations it claims, which assert_populated
    holds to a size.  (A plain scene has one or two clamped rows; a relative L2 over them is one
    fp32 sum's cancellation error, not a bar on a tensor.)"""
    return tuple(dict(edge="beyond", opaque="capped", dark="clamped_sh")[k] for k in claims(c))


def subsets(s, st):
    """Row masks from the oracle's forward state `st` of scene `s`:
      beyond      the view-space mean past 1.3 * tanfov in x or y, and tiles_touched > 0;
      capped      opacity * exp(power) at the nearest pixel centre above 0.99 (float64, from the
                  oracle's xy and conic_opacity);
      clamped_sh  any colour channel clamped;
    and, for assert_populated: `visible`, the per-channel flags `channels` (P, 3) and the fp64
    pre-clamp colour `precolour` (P, 3; None for precomputed colours)."""
    import dense_torch as DT
    import torch
    P, W, H = st["P"], st["W"], st["H"]
    V = st["view"].astype(np.float64).reshape(4, 4)
    m = st["means3D"].astype(np.float64)
    t = m @ V[:3, :3] + V[3, :3]
    vis = (st["radii"] > 0) & (st["tiles_touched"] > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        past = (np.abs(t[:, 0] / t[:, 2]) > 1.3 * float(st["tanfovx"])) | \
               (np.abs(t[:, 1] / t[:, 2]) > 1.3 * float(st["tanfovy"]))
    xy = st["xy"].astype(np.float64)
    co = st["conic_opacity"].astype(np.float64)
    dx = xy[:, 0] - np.clip(np.rint(xy[:, 0]), 0, W - 1)
    dy = xy[:, 1] - np.clip(np.rint(xy[:, 1]), 0, H - 1)
    power = -0.5 * (co[:, 0] * dx * dx + co[:, 2] * dy * dy) - co[:, 1] * dx * dy
    capped = vis & (power <= 0) & (co[:, 3] * np.exp(np.minimum(power, 0.0)) > 0.99)
    channels = st["clamped"].astype(bool).reshape(P, 3) & vis[:, None]
    pre = None
    if st["shs"] is not None:
        d = torch.tensor(m - st["campos"].astype(np.float64))
        d = d / d.norm(dim=1, keepdim=True)
        pre = (DT.eval_sh_t(st["sh_degree"], torch.tensor(st["shs"], dtype=torch.float64), d) + 0.5).numpy()
    return dict(beyond=vis & past, capped=capped, clamped_sh=channels.any(1), visible=vis, channels=channels,
                precolour=pre)


def assert_populated(masks, grads, claimed=("edge", "opaque", "dark")):
    """Every population a case claims is there (`grads`: the oracle's backward)."""
    if "edge" in claimed:
        moved = np.any(grads["dL_dmeans3D"] != 0, axis=1) & masks["beyond"]
        assert int(moved.sum()) >= MIN_BEYOND, ("beyond rows with a position gradient", int(moved.sum()),
                                                int(masks["beyond"].sum()))
    if "opaque" in claimed:
        assert int(masks["capped"].sum()) >= MIN_CAPPED, ("capped rows", int(masks["capped"].sum()))
    if "dark" in claimed:
        vis = masks["visible"]
        share = float(masks["channels"][vis].mean())
        assert MIN_SHARE <= share <= 1.0 - MIN_SHARE, ("clamped channel share", share)
        gap = float(np.abs(masks["precolour"][vis]).min())
        assert gap > COLOUR_GAP, ("a colour channel within 1e-5 of the clamp", gap)
