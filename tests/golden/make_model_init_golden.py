"""Generate model_init.npz from the reference's own GaussianModel.create_from_pcd
(scene/gaussian_model.py:163-278; build container only), the way make_train_golden.py runs
densify_and_prune: the module imported with its native dependencies stubbed, a CPU device shim, and
distCUDA2 replaced by the brute-force kNN of tests/model_init_ref.py (include/gsr_knn.h's
summation order).

  skybox_*    ~200 cloud points, skybox_points = 16, no scaffold_file: the inputs, the two
              torch.rand draws the run consumed (checked bit for bit against a replay of the
              generator), dist2 as the stub returned it, and every parameter the model is left with
  scaffold_*  the same cloud as a chunk behind a 40-row scaffold (3 skybox rows) and a hand-written
              bounds pair: load_ply_file is replaced by a function returning the scaffold's arrays
              in plyfile's layout (plyfile is not installed), pc_info.txt / center.txt / extent.txt
              are real files in a temporary directory

Nothing from the reference is copied; only numbers are kept.
Usage:  python tests/golden/make_model_init_golden.py [--ref /root/reference]
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))


class _Shim:
    """make_golden._NoCuda plus torch.rand / torch.eye without their device, torch.rand recorded."""

    def __init__(self):
        self.draws = []

    def __enter__(self):
        from make_golden import _NoCuda
        self.base = _NoCuda()
        self.base.__enter__()
        self.rand, self.eye = torch.rand, torch.eye

        def rand(*a, **k):
            k.pop("device", None)
            r = self.rand(*a, **k)
            self.draws.append(r.clone())
            return r

        def eye(*a, **k):
            k.pop("device", None)
            return self.eye(*a, **k)
        torch.rand, torch.eye = rand, eye
        return self

    def __exit__(self, *exc):
        torch.rand, torch.eye = self.rand, self.eye
        self.base.__exit__(*exc)


def _model(gm, max_sh_degree):
    m = gm.GaussianModel.__new__(gm.GaussianModel)
    m.setup_functions()
    m.max_sh_degree = max_sh_degree
    m.active_sh_degree = 0
    return m


def _params(m, tag):
    return {f"{tag}_xyz": m._xyz, f"{tag}_f_dc": m._features_dc, f"{tag}_f_rest": m._features_rest,
            f"{tag}_opacity": m._opacity, f"{tag}_scaling": m._scaling, f"{tag}_rotation": m._rotation}


def main(ref):
    import model_init_ref as R
    from make_train_golden import _import_gaussian_model
    gm = _import_gaussian_model(ref)
    rec = {}

    def dist_stub(x):
        d = R.knn_mean_dist2(x.detach().numpy())
        rec["dist2"] = d.copy()
        return torch.from_numpy(d)
    gm.distCUDA2 = dist_stub

    rng = np.random.default_rng(31)
    N, S = 203, 16
    pts = (rng.normal(size=(N, 3)) * [6.0, 4.0, 1.5] + [2.0, -1.0, 0.5]).astype(np.float32)
    col = rng.uniform(0, 1, size=(N, 3)).astype(np.float32)
    pcd = types.SimpleNamespace(points=pts, colors=col)
    cams = [types.SimpleNamespace(image_name=f"im{k}") for k in range(3)]
    out = {"points": pts, "colors": col, "n_images": np.int32(len(cams))}

    # ---- skybox mode, the coarse model (max_sh_degree = 1) ----
    m = _model(gm, 1)
    torch.manual_seed(77)
    state = torch.get_rng_state()
    with _Shim() as shim:
        m.create_from_pcd(pcd, cams, 3.5, S, "", "", False)
    assert len(shim.draws) == 2 and all(d.shape == (S,) for d in shim.draws)
    torch.set_rng_state(state)
    replay = [torch.rand(S), torch.rand(S)]
    assert all(torch.equal(a, b) for a, b in zip(shim.draws, replay)), "the draws are not two torch.rand(S)"
    out.update(skybox_points=np.int32(m.skybox_points), u_theta=shim.draws[0].numpy(), u_phi=shim.draws[1].numpy(),
               skybox_dist2=rec["dist2"])
    out.update({k: v.detach().numpy().copy() for k, v in _params(m, "skybox").items()})

    # ---- a chunk behind a scaffold (max_sh_degree = 3) ----
    Ps, Ssc = 40, 3
    sc_xyz = (rng.uniform(-1, 1, size=(Ps, 3)) * [40.0, 40.0, 5.0]).astype(np.float32)
    sc = dict(xyz=sc_xyz, shs=rng.normal(size=(Ps, 4, 3)).astype(np.float32),
              opacity=rng.normal(size=(Ps, 1)).astype(np.float32),
              scaling=(rng.normal(size=(Ps, 3)) - 2).astype(np.float32),
              rotation=rng.normal(size=(Ps, 4)).astype(np.float32))
    center, extent = [1.5, -2.25, 0.0], [20.0, 12.0, 9.0]

    def load_ply_file(path, degree):  # plyfile's layout: f_dc (P, 3, 1), f_extra (P, 3, 3), float64
        assert degree == 1 and path.endswith("/point_cloud.ply")
        f = sc["shs"].astype(np.float64)
        return (sc["xyz"].astype(np.float64), f[:, :1].transpose(0, 2, 1).copy(), f[:, 1:].transpose(0, 2, 1).copy(),
                sc["opacity"].astype(np.float64), sc["scaling"].astype(np.float64), sc["rotation"].astype(np.float64))
    m = _model(gm, 3)
    m.load_ply_file = load_ply_file
    with tempfile.TemporaryDirectory() as tmp:
        sdir, bdir = os.path.join(tmp, "scaffold"), os.path.join(tmp, "bounds")
        os.makedirs(sdir)
        os.makedirs(bdir)
        open(os.path.join(sdir, "pc_info.txt"), "w").write(str(Ssc))
        open(os.path.join(bdir, "center.txt"), "w").write(" ".join(repr(v) for v in center))
        open(os.path.join(bdir, "extent.txt"), "w").write(" ".join(repr(v) for v in extent))
        with _Shim() as shim:
            m.create_from_pcd(pcd, cams, 3.5, S, sdir, bdir, False)  # skybox_points overridden to 0
    assert not shim.draws
    out.update({"scaffold_in_" + k: v for k, v in sc.items()})
    out.update(scaffold_skybox_points=np.int32(m.skybox_points), scaffold_points=np.int32(m.scaffold_points),
               center=np.array(center, np.float32), extent=np.array(extent, np.float32), scaffold_dist2=rec["dist2"])
    out.update({k: v.detach().numpy().copy() for k, v in _params(m, "scaffold").items()})
    np.savez_compressed(os.path.join(OUT, "model_init.npz"), **out)
    print("wrote model_init.npz: skybox rows", out["skybox_xyz"].shape[0], "scaffold rows", out["scaffold_xyz"].shape[0],
          "scaffold_points", int(m.scaffold_points))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    a = ap.parse_args()
    sys.path.insert(0, a.ref)
    main(a.ref)
