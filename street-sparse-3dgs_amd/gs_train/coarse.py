"""The coarse scaffold stage: train_coarse.py:59-148 on the existing kernels, SH degree 1 (M = 4).

CoarseTrainStep is one iteration, free of host synchronisation (the reference's .item() feeds only
its progress bar):

  1. learning rates: train_coarse.py never calls update_learning_rate; the xyz group's rate is 0
     for the whole run (:55-57) -- its moments still advance -- and every other rate stays at its
     initial value
  2. render_coarse (gaussian_renderer/__init__.py:306-417): no depth output, no exposure affine and
     no clamp, a fresh torch.rand(3) background; `debug` is an option here (the reference forces
     it on, INTEGRATION.md says what that costs)
  3. image * alpha_mask when the view has a mask, then (1 - lambda) L1 + lambda (1 - SSIM) (:98-105)
  4. max_radii2D = max(max_radii2D, radii) on the visible rows (:110); xyz_gradient_accum and denom
     stay untouched
  5. _scaling.grad[:skybox] = 0 only (:132): unlike train_single.py the skybox rows' other
     parameters train
  6. optimizer.step((opacity.grad != 0).nonzero()) (:133-134).  That (R, 2) index of the (P, 1)
     gradient also updates row 0 whenever any row is relevant, and no relevant row
     at all means the dense update.  Without the nonzero(): the relevance handed to the fused Adam
     is the opacity gradient with element 0 replaced by max |gradient| -- nonzero exactly when some
     row is relevant.  Then zero_grad(set_to_none=True)
  7. shrink_scales(_scaling, 0.1 * cameras_extent, first_row=skybox) (:141-145)

TrainCoarse is the loop around it: one more SH degree every sh_interval iterations up to degree 1,
checkpoints (gs_train.chunk.capture / restore), and save() -> gs_train.scaffold.save_scaffold."""
from __future__ import annotations

import torch

from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer

from .activations import shrink_scales
from .chunk import capture, restore  # noqa: F401  (the stage's checkpoints are the chunk stage's)
from .harness import LR, TrainStep
from .scaffold import save_scaffold


class CoarseTrainStep(TrainStep):
    """cameras, gts, alpha_masks, skybox_points, cameras_extent: as TrainStep.  The coarse stage has
    no depth supervision, no depth-only views and no scaffold of its own; the keywords are accepted
    (gs_train.harness.make_problem passes them) and must be empty."""

    def __init__(self, gaussians, cameras, gts, W, H, cameras_extent=10.0, mono_invdepths=None, depth_masks=None,
                 alpha_masks=None, skybox_points=0, scaffold_points=0, iterations=LR["iterations"], depth_only=None,
                 debug=False):
        if mono_invdepths is not None or depth_masks is not None or (depth_only is not None and any(depth_only)):
            raise ValueError("the coarse stage has no depth supervision (train_coarse.py:98-105)")
        if scaffold_points:
            raise ValueError("the coarse stage trains the scaffold: it has none of its own")
        super().__init__(gaussians, cameras, gts, W, H, cameras_extent=cameras_extent, alpha_masks=alpha_masks,
                         skybox_points=skybox_points, iterations=iterations)
        self.debug = bool(debug)
        for pg in self.optimizer.param_groups:
            if pg["name"] == "xyz":
                pg["lr"] = 0.0  # train_coarse.py:55-57

    def render(self, cam_idx, bg):
        c = self.cams[cam_idx]
        g = self.g
        rs = GaussianRasterizationSettings(
            image_height=self.H, image_width=self.W, tanfovx=c["tx"], tanfovy=c["ty"], bg=bg, scale_modifier=1.0,
            viewmatrix=c["view"], projmatrix=c["proj"], sh_degree=g.active_sh_degree, campos=c["campos"],
            prefiltered=False, debug=self.debug, do_depth=False, render_indices=self.empty_i,
            parent_indices=self.empty_i, interpolation_weights=self.empty_f, num_node_kids=self.empty_id)
        means2D = self._means2D_leaf()
        scales, rotations, opacities = self._activations()
        color, radii, invd = GaussianRasterizer(rs)(means3D=g.get_xyz, means2D=means2D, shs=g.get_features,
                                                    colors_precomp=None, opacities=opacities, scales=scales,
                                                    rotations=rotations, cov3D_precomp=None)
        return color, invd, means2D, radii

    def _densify_stats(self, radii, grad2d):
        m = self.g.max_radii2D  # radii >= 0 and 0 on the invisible rows: the maximum over every row is :110
        torch.maximum(m, radii.to(m.dtype), out=m)

    def _lock_skybox(self):
        self.g._scaling.grad[:self.skybox] = 0

    def _sparse_step(self):
        rel = self.g._opacity.grad.detach().reshape(-1).clone()
        if rel.numel():
            rel[0] = rel.abs().amax()
        self.optimizer.step(relevance=rel)

    def _shrink(self):
        shrink_scales(self.g._scaling, self.extent * 0.1, first_row=self.skybox)

    def step(self, cam_idx=None, before_update=None):
        """One iteration; returns the loss tensor (no host synchronisation).  before_update: called
        between the statistics and the optimizer, where train_coarse.py saves (:120-122)."""
        g = self.g
        k = self._view(cam_idx)
        bg = torch.rand(3, device=g._xyz.device)
        image, _, means2D, radii = self.render(k, bg)
        if self.amask[k] is not None:
            image = image * self.amask[k]
        loss = self._photo_loss(image, self.gts[k])
        self._backward(loss)
        with torch.no_grad():
            self._densify_stats(radii, means2D.grad)
            if before_update is not None:
                before_update()
            if self.skybox > 0:
                self._lock_skybox()
            self._sparse_step()
            self.optimizer.zero_grad(set_to_none=True)
            self._shrink()
        self.iteration += 1
        return loss.detach()


class TrainCoarse:
    """train_coarse.py's loop around a CoarseTrainStep.  The reference's last iteration renders but
    updates nothing (:124-127): run() stops after iterations - 1 updates, as TrainChunk does.
    on_checkpoint: callable(iteration, capture dict); on_save: callable(iteration) -> the directory
    save() writes that iteration's scaffold to."""

    def __init__(self, step, iterations=30_000, sh_interval=1000, max_sh_degree=1, checkpoint_iterations=(),
                 save_iterations=(), on_checkpoint=None, on_save=None):
        self.ts = step
        self.iterations = int(iterations)
        self.sh_interval = int(sh_interval)
        self.max_sh_degree = int(max_sh_degree)
        if (self.max_sh_degree + 1) ** 2 > step.g.get_features.shape[1]:
            raise ValueError("max_sh_degree: the model holds fewer SH coefficients")
        self.checkpoint_iterations = tuple(checkpoint_iterations)
        self.save_iterations = tuple(save_iterations)
        self.on_checkpoint = on_checkpoint
        self.on_save = on_save

    def iteration(self):
        ts = self.ts
        it = ts.iteration
        if it % self.sh_interval == 0 and ts.g.active_sh_degree < self.max_sh_degree:
            ts.g.active_sh_degree += 1  # oneupSHdegree (:87-88)
        saving = it in self.save_iterations and self.on_save is not None
        loss = ts.step(before_update=(lambda: self.save(self.on_save(it))) if saving else None)
        if it in self.checkpoint_iterations and self.on_checkpoint is not None:
            self.on_checkpoint(it, capture(ts))
        return loss

    def run(self, until=None, callback=None):
        """Iterations from the step's current one up to `until` (default: iterations - 1).
        callback(iteration, loss tensor) after each."""
        last = self.iterations - 1 if until is None else until
        while self.ts.iteration <= last:
            it = self.ts.iteration
            loss = self.iteration()
            if callback is not None:
                callback(it, loss)

    def save(self, dir) -> None:
        save_scaffold(dir, self.ts.g, self.ts.skybox)
