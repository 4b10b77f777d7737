"""train_coarse.py:94-145 in the reference's formulation, in plain torch ops, for
tests/test_gpu_coarse.py: the split SH layout, the get_* activations, conv2d SSIM, the
(opacity.grad != 0).nonzero() index -- an (R, 2) tensor whose second column is all 0, so OurAdam's
gather / scatter also updates row 0 -- handed to Adam.step(relevant), the boolean-mask scale shrink.
The pieces are oracle/train_torch_ref.py's, by import."""
from __future__ import annotations

import torch

from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer


def reference_coarse_step_cls():
    from gs_train.harness import LR
    from train_torch_ref import ReferenceTrainStep, photo_loss

    class ReferenceCoarseStep(ReferenceTrainStep):
        def __init__(self, gaussians, cameras, gts, W, H, cameras_extent=10.0, alpha_masks=None, skybox_points=0,
                     iterations=LR["iterations"], **unused):
            assert not unused.get("mono_invdepths") and not unused.get("scaffold_points")
            super().__init__(gaussians, cameras, gts, W, H, cameras_extent=cameras_extent, alpha_masks=alpha_masks,
                             skybox_points=skybox_points, iterations=iterations)
            for pg in self.optimizer.param_groups:  # train_coarse.py:55-57
                if pg["name"] == "xyz":
                    pg["lr"] = 0.0

        def step(self, cam_idx=None):
            g = self.g
            k = self._view(cam_idx)
            c = self.cams[k]
            bg = torch.rand(3, device=g._xyz.device)  # :62
            # render_coarse (gaussian_renderer/__init__.py:306-417): no depth, no exposure
            rs = GaussianRasterizationSettings(
                image_height=self.H, image_width=self.W, tanfovx=c["tx"], tanfovy=c["ty"], bg=bg, scale_modifier=1.0,
                viewmatrix=c["view"], projmatrix=c["proj"], sh_degree=g.active_sh_degree, campos=c["campos"],
                prefiltered=False, debug=False, do_depth=False, render_indices=self.empty_i,
                parent_indices=self.empty_i, interpolation_weights=self.empty_f, num_node_kids=self.empty_id)
            means2D = torch.zeros_like(g._xyz, requires_grad=True) + 0
            image, radii, _ = GaussianRasterizer(rs)(means3D=g.get_xyz, means2D=means2D, shs=g.get_features,
                                                     colors_precomp=None, opacities=g.get_opacity,
                                                     scales=g.get_scaling, rotations=g.get_rotation, cov3D_precomp=None)
            if self.amask[k] is not None:  # :99-105
                image = image * self.amask[k]
            loss = photo_loss(image, self.gts[k], LR["lambda_dssim"])
            loss.backward()
            vis = radii > 0
            g.max_radii2D[vis] = torch.max(g.max_radii2D[vis], radii[vis].float())  # :110
            with torch.no_grad():
                g._scaling.grad[:self.skybox, :] = 0  # :132
                relevant = (g._opacity.grad != 0).nonzero()  # :133, shape (R, 2)
                self.last_relevant = relevant
                self.optimizer.step(relevant)
                self.optimizer.zero_grad(set_to_none=True)
                vals, _ = g.get_scaling.max(dim=1)  # :141-145
                violators = vals > self.extent * 0.1
                violators[:self.skybox] = False
                g._scaling[violators] = torch.log(g.get_scaling[violators] * 0.8)
            self.iteration += 1
            return loss.detach()

    return ReferenceCoarseStep
