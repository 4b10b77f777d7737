"""Generate tests/golden/eval.npz from the reference's own evaluation functions (build container only).

For (H, W) = (7, 9) (smaller than the window), (16, 16), (37, 53) (ragged) and (70, 130) (several
tiles both ways): an unclamped image and target, an alpha mask with about 10% zeros, a predicted and
a target inverse depth map in [0, 0.4), and five regions: the three depth ranges of
render_hierarchy_final.py:31-35 (get_depth_range_mask on the fp32 target depth), one block that
straddles tile borders and the single pixel (0, 0).  Stored per case and row (row 0 the whole image,
then the regions): psnr, ssim, imae, irmse and the weight as render_hierarchy_final.py's
compute_metrics / compute_depth_metrics return them on fp32 tensors (`ref32`), and the same functions
on the same inputs cast to fp64 (`ref64`; the masks stay the fp32 ones).  The module is imported with
its heavy imports stubbed (lpips returns 0); utils/loss_utils.py and utils/image_utils.py are the
reference's own.

D_other / D_single: the largest |ref32 - ref64| over all cases and rows of a kind (one-pixel regions /
every other row) for psnr (dB), ssim, imae and irmse (relative): the reference's own fp32 error, from
which the tests take their tolerances.

The generator asserts what makes the reference unambiguous on these inputs: every nonzero window
weight is >= 1.05e-6 (the threshold is 1e-6; the smallest possible weight is the squared corner tap,
1.0576e-6) and every SSIM denominator in a valid window is >= 1e-8 (the threshold is 1e-10).

Nothing from the reference is copied; only numbers are kept.
Usage:  python tests/golden/make_eval_golden.py --ref <reference checkout>
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import eval_ref  # noqa: E402  (only for the assertions on window weights and denominators)

SIZES = [(7, 9), (16, 16), (37, 53), (70, 130)]


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def import_reference(ref):
    """render_hierarchy_final.py with the reference's utils and everything heavy stubbed."""
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    stub("utils")
    load_by_path("utils.loss_utils", os.path.join(ref, "utils", "loss_utils.py"))
    load_by_path("utils.image_utils", os.path.join(ref, "utils", "image_utils.py"))
    stub("gaussian_renderer", render_post=None)
    stub("scene", Scene=None, GaussianModel=None)
    stub("tqdm", tqdm=lambda it, **kw: it)
    stub("arguments", ModelParams=None, PipelineParams=None, OptimizationParams=None)
    tv = stub("torchvision")
    tv.io = stub("torchvision.io")
    stub("lpipsPyTorch", lpips=lambda a, b, **kw: torch.zeros(()))
    stub("gaussian_hierarchy")
    stub("gaussian_hierarchy._C", expand_to_size=None, get_interpolation_weights=None)
    return load_by_path("ref_render_hierarchy_final", os.path.join(ref, "render_hierarchy_final.py"))


def rows_of(R, image, gt, alpha, invd, gt_invd, masks):
    """(1 + len(masks), 5): psnr, ssim, imae, irmse, weight as render_set computes them (:282-313)."""
    out = []
    p, s, _ = R.compute_metrics(image, gt, alpha, segmentation_mask=None)
    i1, i2 = R.compute_depth_metrics(invd, gt_invd, alpha)
    out.append([p.item(), s.item(), i1.item(), i2.item(), float(alpha.numel())])
    for m in masks:
        assert torch.sum(m) > 0
        p, s, _ = R.compute_metrics(image, gt, alpha, segmentation_mask=m)
        i1, i2 = R.compute_depth_metrics(invd, gt_invd, alpha * m)
        out.append([p.item(), s.item(), i1.item(), i2.item(), float(torch.sum((m * alpha) > 0).item())])
    return np.array(out, np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout")
    R = import_reference(ap.parse_args().ref)
    g = torch.Generator().manual_seed(23)
    out = {"n": np.int32(len(SIZES))}
    D = {"single": np.zeros(4), "other": np.zeros(4)}
    min_w, min_den = np.inf, np.inf
    win = eval_ref.window(torch.float32)
    for k, (H, W) in enumerate(SIZES):
        raw = torch.rand((3, H, W), generator=g) * 1.3 - 0.15  # some values outside [0, 1]
        raw_gt = raw + 0.12 * torch.randn((3, H, W), generator=g)
        # the single-pixel region: inside [0, 1], visible and different in every channel (finite PSNR)
        raw[:, 0, 0] = 0.3 + 0.4 * torch.rand(3, generator=g)
        raw_gt[:, 0, 0] = raw[:, 0, 0] + 0.02 + 0.1 * torch.rand(3, generator=g)
        alpha = (torch.rand((1, H, W), generator=g) >= 0.1).float()
        alpha[0, 0, 0] = 1.0
        gt_invd = torch.rand((1, H, W), generator=g) * 0.4
        invd = (gt_invd + 0.03 * torch.randn((1, H, W), generator=g)).clamp(min=0.0)
        masks = [R.get_depth_range_mask(gt_invd, lo, hi) for _, lo, hi in R.DEPTH_RANGES]
        block = torch.zeros((1, H, W))
        r0, c0 = H // 7, W // 3
        block[:, r0:r0 + max(2, H // 2), c0:c0 + max(2, W // 2)] = 1.0
        single = torch.zeros((1, H, W))
        single[0, 0, 0] = 1.0
        masks += [block, single]
        kinds = ["other"] * 5 + ["single"]
        image, gt = raw.clamp(0.0, 1.0), raw_gt.clamp(0.0, 1.0)  # render_set clamps both (:259-262)
        ref32 = rows_of(R, image, gt, alpha, invd, gt_invd, masks)
        d = lambda t: t.double()
        # ssim_masked convolves mask.float() whatever the images' dtype: for the fp64 evaluation its
        # conv2d casts the input to the window's dtype (exact for a 0/1 mask)
        lu = sys.modules["utils.loss_utils"]
        real_F = lu.F
        lu.F = types.SimpleNamespace(conv2d=lambda x, w, **kw: real_F.conv2d(x.to(w.dtype), w, **kw))
        try:
            ref64 = rows_of(R, d(image), d(gt), d(alpha), d(invd), d(gt_invd), [d(m) for m in masks])
        finally:
            lu.F = real_F
        assert np.array_equal(ref32[:, 4], ref64[:, 4]) and np.isfinite(ref64).all(), (ref32, ref64)
        for r, kind in enumerate(kinds):
            e = np.abs(ref32[r, :4] - ref64[r, :4])
            e[2:] /= np.abs(ref64[r, 2:4])
            D[kind] = np.maximum(D[kind], e)
        for m in masks:  # the conditions under which the reference's thresholds decide nothing
            w, valid, _, den = eval_ref.masked_ssim_terms(image * alpha, gt * alpha, m, win)
            min_w = min(min_w, float(w[w > 0].min()))
            min_den = min(min_den, float(den[valid].min()))
        bits = torch.zeros((H, W), dtype=torch.int32)
        for r, m in enumerate(masks):
            bits |= m[0].to(torch.int32) << r
        out.update({f"image_{k}": raw.numpy(), f"gt_{k}": raw_gt.numpy(), f"alpha_{k}": alpha[0].numpy(),
                    f"invdepth_{k}": invd[0].numpy(), f"gt_invdepth_{k}": gt_invd[0].numpy(),
                    f"bits_{k}": bits.numpy().astype(np.uint16), f"ref32_{k}": ref32, f"ref64_{k}": ref64,
                    f"single_{k}": np.array([kd == "single" for kd in kinds])})
    assert min_w >= 1.05e-6, f"a window weight of {min_w} is too close to the 1e-6 threshold"
    assert min_den >= 1e-8, f"an SSIM denominator of {min_den} is too close to the 1e-10 threshold"
    out["D_single"], out["D_other"] = D["single"], D["other"]
    out["min_window_weight"], out["min_denominator"] = np.float64(min_w), np.float64(min_den)
    path = os.path.join(OUT, "eval.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1_000_000
    print(f"{path}: {os.path.getsize(path)} bytes; D_other {D['other']}; D_single {D['single']}; "
          f"min window weight {min_w:.4e}; min denominator {min_den:.3e}")


if __name__ == "__main__":
    main()
