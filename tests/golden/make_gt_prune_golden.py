"""Generate densify_prune_gt_<case>.npz: the reference's own GaussianModel.densify_and_prune with
gt_point_cloud_constraints on (scene/gaussian_model.py:733-778 calling compare_points_to_gt,
:853-962), on the seeded 1200-row models of make_train_golden.make_densify_prune (cases "plain" and
"scaffold" with 150 fixed rows), build container only.

The model's gt_point_cloud is a stub whose .search(x, 1) returns the float32 all-pairs squared
distances of tests/gt_ref.py (FAISS's own rounding is not defined; the project's d2 rule is), over a
cloud of 4000 points; constraint_treshold is of the order of the cloud's spacing and the four XY
bounds are set as load_gt_point_cloud sets them.  The inputs are those of densify_prune_<case>.npz, array for array
(checked here), and are read from that file, which keeps this one under the size limit of a committed
file.  Besides the standard-normal draws behind the split samples and every parameter, moment and
statistic left, the fixture keeps the cloud, the threshold and what compare_points_to_gt saw and returned:
the positions at that moment, the opacity-prune mask, the protected (split children) mask, the
combined mask, and the two counts.

The generator refuses to write a fixture unless
  - no checked row's minimum d2, evaluated in fp64, lies within 1e-4 relative of thr^2,
  - an old row, a clone and (scaffold) a row below 150 are distance-pruned,
  - a far split child is protected, a far row outside the XY bounds is kept, and a row already
    opacity-pruned is also far.

Nothing from the reference is copied; only numbers are kept.
Usage:  python tests/golden/make_gt_prune_golden.py --ref <checkout of the reference>
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))

import gt_ref  # noqa: E402  (tests/gt_ref.py)
from make_golden import _NoCuda  # noqa: E402
from make_train_golden import _import_gaussian_model  # noqa: E402

G_CLOUD = 4000
THR = 0.8  # the cloud below has one point per ~1.5 m^3: spacing ~1.15


def make_cloud(seed):
    """4000 points uniform in [-8, 8] x [-8, 8] x [-12, 12]: the model's positions (N(0, 5^2) per
    axis) fall inside and outside its XY bounds, near and far from its points."""
    rng = np.random.default_rng(seed)
    lo = np.array([-8.0, -8.0, -12.0])
    return (lo + rng.random((G_CLOUD, 3)) * (-2.0 * lo)).astype(np.float32)


class _FlatIndexStub:
    """gt_point_cloud.search(x, 1) as the d2 rule gives it: float32 all-pairs, every point scanned."""

    def __init__(self, cloud):
        self.cloud = cloud

    def search(self, x, k):
        assert k == 1 and x.dtype == np.float32
        d = gt_ref.min_d2(x, self.cloud)
        return d[:, None], np.zeros((x.shape[0], 1), np.int64)


def min_d2_fp64(xyz, cloud):
    p, c = xyz.astype(np.float64), cloud.astype(np.float64)
    out = np.empty(p.shape[0])
    for s in range(0, p.shape[0], 256):
        d = c[None] - p[s:s + 256, None]
        out[s:s + 256] = (d * d).sum(-1).min(1)
    return out


def make(ref):
    gm = _import_gaussian_model(ref)
    our_adam = sys.modules["scene.OurAdam"]
    for case, scaffold in (("plain", None), ("scaffold", 150)):
        # the seeded model of make_train_golden.make_densify_prune, draw for draw
        g = torch.Generator().manual_seed(21 if scaffold is None else 22)
        P = 1200
        m = gm.GaussianModel.__new__(gm.GaussianModel)
        m.setup_functions()
        q = torch.randn((P, 4), generator=g)
        init = {"xyz": torch.randn((P, 3), generator=g) * 5, "f_dc": torch.randn((P, 1, 3), generator=g),
                "f_rest": torch.randn((P, 15, 3), generator=g), "opacity": torch.randn((P, 1), generator=g) * 2,
                "scaling": torch.randn((P, 3), generator=g) * 0.7 - 4.0, "rotation": q}
        for k, v in init.items():
            setattr(m, "_" + ("features_dc" if k == "f_dc" else "features_rest" if k == "f_rest" else k),
                    torch.nn.Parameter(v.clone()))
        acc = torch.rand((P, 1), generator=g) * 0.001
        acc[::97] = float("nan")
        maxr = torch.rand(P, generator=g) * 20
        m.xyz_gradient_accum = acc.clone()
        m.xyz_gradient_accum_depth = torch.zeros((P, 1))
        m.denom = torch.randint(0, 5, (P, 1), generator=g).float()
        m.max_radii2D = maxr.clone()
        m.percent_dense = 0.0001
        m.scaffold_points = scaffold
        attr = {"xyz": m._xyz, "f_dc": m._features_dc, "f_rest": m._features_rest, "opacity": m._opacity,
                "scaling": m._scaling, "rotation": m._rotation}
        m.optimizer = our_adam.Adam([{"params": [attr[n]], "lr": 0.0, "name": n} for n in attr], lr=0.0, eps=1e-15)
        out = {"in_" + n: v.numpy() for n, v in init.items()}
        for n, p_ in attr.items():
            mom, var = torch.randn(p_.shape, generator=g), torch.rand(p_.shape, generator=g)
            m.optimizer.state[p_] = {"step": torch.tensor(7.0), "exp_avg": mom.clone(), "exp_avg_sq": var.clone()}
            out["in_m_" + n], out["in_v_" + n] = mom.numpy(), var.numpy()
        out.update(in_accum=acc.numpy(), in_max_radii2D=maxr.numpy(), in_denom=m.denom.numpy())
        args = dict(max_grad=0.0002, min_opacity=0.05, extent=200.0)

        # the constraint, set up as load_gt_point_cloud leaves the model
        cloud = make_cloud(31 if scaffold is None else 32)
        m.gt_point_cloud = _FlatIndexStub(cloud)
        m.constraint_treshold = THR
        m.gt_x_min, m.gt_x_max = np.min(cloud[:, 0]), np.max(cloud[:, 0])
        m.gt_y_min, m.gt_y_max = np.min(cloud[:, 1]), np.max(cloud[:, 1])

        real_normal, rec = torch.normal, {}

        def normal(*a, **k):
            r = real_normal(*a, **k)
            rec["samples"], rec["std"] = r.clone(), k["std"].clone()
            return r
        real_compare = m.compare_points_to_gt

        def compare(existing_mask=None, protected_mask=None):
            rec["cmp_xyz"] = m.get_xyz.detach().clone().numpy()
            rec["cmp_existing"] = existing_mask.clone().numpy()
            rec["cmp_protected"] = protected_mask.clone().numpy()
            r = real_compare(existing_mask, protected_mask)
            rec["cmp_mask"] = r.clone().numpy()
            return r
        m.compare_points_to_gt = compare
        torch.manual_seed(1234)
        state = torch.get_rng_state()
        torch.normal = normal
        try:
            with _NoCuda():
                m.densify_and_prune(args["max_grad"], args["min_opacity"], args["extent"], True)
        finally:
            torch.normal = real_normal
        torch.set_rng_state(state)
        z = torch.empty(rec["samples"].shape).normal_()
        assert torch.equal(z * rec["std"], rec["samples"]), "torch.normal is not normal_() * std here"
        out["normals"] = z.numpy()

        # ---- the conditions a fixture must meet (not tolerances: refuse to write otherwise) ----
        xyz, existing, protected, mask = rec["cmp_xyz"], rec["cmp_existing"], rec["cmp_protected"], rec["cmp_mask"]
        n_split = int(protected.sum()) // 2
        n_old = P - n_split
        n_clone = xyz.shape[0] - n_old - 2 * n_split
        assert n_clone > 0 and n_split > 0 and protected[n_old + n_clone:].all() and not protected[:n_old + n_clone].any()
        inside = gt_ref.inside_bounds(xyz, cloud)
        checked = inside & ~existing & ~protected
        d64 = min_d2_fp64(xyz, cloud)
        rel = np.abs(d64[checked] / (THR * THR) - 1.0)
        assert rel.min() > 1e-4, f"{case}: a checked row's min d2 is within {rel.min():.2e} relative of thr^2"
        far64 = d64 > THR * THR
        dist_pruned = mask & ~existing
        assert np.array_equal(dist_pruned, checked & far64), f"{case}: the reference's mask is not the rule's"
        is_old = np.arange(xyz.shape[0]) < n_old
        is_clone = (np.arange(xyz.shape[0]) >= n_old) & ~protected
        assert (dist_pruned & is_old).any(), f"{case}: no distance-pruned old row"
        assert (dist_pruned & is_clone).any(), f"{case}: no distance-pruned clone"
        assert (protected & inside & far64 & ~existing).any(), f"{case}: no far, protected split child"
        assert (~inside & far64 & ~mask).any(), f"{case}: no far row outside the XY bounds that is kept"
        assert (existing & inside & far64).any(), f"{case}: no opacity-pruned row that is also far"
        n_fixed = int(dist_pruned[:scaffold or 0].sum())
        if scaffold:
            assert n_fixed > 0, f"{case}: no distance-pruned row below {scaffold}"

        out.update(max_grad=np.float32(args["max_grad"]), min_opacity=np.float32(args["min_opacity"]),
                   extent=np.float32(args["extent"]), percent_dense=np.float32(m.percent_dense),
                   scaffold=np.int32(scaffold or 0), cloud=cloud, threshold=np.float64(THR),
                   bounds=np.array([m.gt_x_min, m.gt_x_max, m.gt_y_min, m.gt_y_max], np.float32),
                   cmp_xyz=xyz, cmp_existing=existing, cmp_protected=protected, cmp_mask=mask,
                   gt_pruned=np.int64(dist_pruned.sum()), gt_pruned_fixed=np.int64(n_fixed))
        final = {"xyz": m._xyz, "f_dc": m._features_dc, "f_rest": m._features_rest, "opacity": m._opacity,
                 "scaling": m._scaling, "rotation": m._rotation}
        grp = {pg["name"]: pg["params"][0] for pg in m.optimizer.param_groups}
        for n, p_ in final.items():
            assert grp[n] is p_
            st = m.optimizer.state[p_]
            out["out_" + n] = p_.detach().numpy()
            out["out_m_" + n], out["out_v_" + n] = st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
        out.update(out_accum=m.xyz_gradient_accum.numpy(), out_denom=m.denom.numpy(),
                   out_max_radii2D=m.max_radii2D.numpy())
        # the inputs live in densify_prune_<case>.npz (same seeds, same draws)
        base = np.load(os.path.join(OUT, f"densify_prune_{case}.npz"))
        for k in [k for k in out if k.startswith("in_")]:
            assert np.array_equal(out[k], base[k], equal_nan=True), f"{case}: {k} differs from densify_prune_{case}.npz"
            del out[k]
        for k in ("max_grad", "min_opacity", "extent", "percent_dense", "scaffold"):
            assert out[k] == base[k]
        np.savez_compressed(os.path.join(OUT, f"densify_prune_gt_{case}.npz"), **out)
        print(case, "P", P, "->", m._xyz.shape[0], "clones", n_clone, "split", n_split, "distance-pruned",
              int(dist_pruned.sum()), "below scaffold", n_fixed, "closest margin", float(rel.min()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    a = ap.parse_args()
    sys.path.insert(0, a.ref)
    make(a.ref)
