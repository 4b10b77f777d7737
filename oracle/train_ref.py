"""TEST INFRASTRUCTURE ONLY -- CPU restatement of the train-step pieces around the rasterizer.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module; the
product (street-sparse-3dgs_amd/gs_train) runs the gfx950 kernels in csrc/loss.hip / optim.hip and never
touches it.  Pinned against tests/golden/{loss,adam,densify}.npz, which
tests/golden/make_train_golden.py produced by running the reference's own functions.

  l1(img, gt)                 utils/loss_utils.py:17-18
  ssim(img, gt)               utils/loss_utils.py:23-58: an 11x11 window (outer product of a
                              normalised sigma-1.5 Gaussian), five depthwise conv2d with zero
                              padding 5, mean of the SSIM map
  photo_loss(img, gt, lam)    train_single.py:121-123
  sparse_adam(...)            scene/OurAdam.py:105-175 + _single_tensor_adam (:249-337) and the
                              _single_tensor_adam2 dense branch (:338-...) when nothing is relevant
  densify_stats(...)          train_single.py:193 + scene/gaussian_model.py:780-793
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

C1 = 0.01 ** 2
C2 = 0.03 ** 2


def window(size: int = 11, sigma: float = 1.5, dtype=torch.float32) -> torch.Tensor:
    g = torch.tensor([math.exp(-((i - size // 2) ** 2) / (2.0 * sigma * sigma)) for i in range(size)],
                     dtype=torch.float32)
    g = g / g.sum()
    return torch.outer(g, g).to(dtype)


def l1(img: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    return (img - gt).abs().mean()


def ssim(img: torch.Tensor, gt: torch.Tensor, size: int = 11) -> torch.Tensor:
    C = img.shape[-3]
    w = window(size, dtype=img.dtype).expand(C, 1, size, size).contiguous()

    def blur(t):
        return F.conv2d(t, w, padding=size // 2, groups=C)

    mu1, mu2 = blur(img), blur(gt)
    s11 = blur(img * img) - mu1 * mu1
    s22 = blur(gt * gt) - mu2 * mu2
    s12 = blur(img * gt) - mu1 * mu2
    num = (2 * mu1 * mu2 + C1) * (2 * s12 + C2)
    den = (mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2)
    return (num / den).mean()


def photo_loss(img, gt, lambda_dssim: float = 0.2):
    return (1.0 - lambda_dssim) * l1(img, gt) + lambda_dssim * (1.0 - ssim(img, gt))


def sparse_adam(params, grads, exp_avgs, exp_avg_sqs, steps, lrs, relevance, beta1=0.9, beta2=0.999, eps=1e-15):
    """One OurAdam step over parallel lists of (P, ...) tensors, in place.  `steps` is a list of
    python step counters (returned incremented).  Rows with relevance != 0 are updated; with no
    such row every row is (the dense branch)."""
    rel = (relevance.flatten() != 0).nonzero().flatten()
    dense = rel.numel() == 0
    new_steps = []
    for p, g, m, v, st, lr in zip(params, grads, exp_avgs, exp_avg_sqs, steps, lrs):
        st = st + 1
        new_steps.append(st)
        idx = slice(None) if dense else rel
        gg, mm, vv, pp = g[idx], m[idx], v[idx], p[idx]
        mm = mm * beta1 + (1 - beta1) * gg
        vv = vv * beta2 + (1 - beta2) * gg * gg
        step_size = lr / (1 - beta1 ** st)
        bc2 = math.sqrt(1 - beta2 ** st)
        denom = vv.sqrt() / bc2 + eps
        pp = pp - step_size * (mm / denom)
        m[idx], v[idx], p[idx] = mm, vv, pp
    return new_steps


def densify_stats(radii, grad2d, max_radii2D, grad_accum, denom):
    vis = radii > 0
    max_radii2D[vis] = torch.max(max_radii2D[vis], radii[vis].to(max_radii2D.dtype))
    n = torch.norm(grad2d[vis, :2], dim=-1, keepdim=True)
    grad_accum[vis] = torch.max(n, grad_accum[vis])
    denom[vis] += 1
