"""LPIPS (VGG16, v0.1) restated in plain torch: the checker of csrc/lpips.hip and gs_train/lpips.py --
test infrastructure, as tests/eval_ref.py is for the other metrics.  Dtype-generic, so it runs in fp64.

The formulation (include/gsr_lpips.h; lpipsPyTorch/modules/lpips.py:32-66, networks.py:41-63,
utils.py:6-8): z-score the two images, run the VGG16 trunk on each, take the ReLU'd activations after
conv 1_2, 2_2, 3_3, 4_3 and 5_3, divide each pixel's channel vector by (its norm + 1e-10), square the
difference, weigh the channels with the stage's linear layer, and average over the pixels -- all of
them, or those of a region's mask resized to the stage with the nearest-neighbour rule.  The head
runs once per region, as the reference's does; the trunk's features are shared (the reference
recomputes them per call, with the same result).

make_weights(seed) stands in for the real weights (59 MB, not committable): VGG16-shaped tensors from
numpy's frozen legacy stream.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

STAGE_CONVS = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
STAGE_CHANNELS = (64, 128, 256, 512, 512)
MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)


def make_weights(seed: int = 0):
    """(vgg, lin): torchvision-style `features.N.weight` / `features.N.bias` and LPIPS-file-style
    `linK.model.1.weight`, fp32.  He-scaled normal convolution weights keep the activations O(1)
    through the 13 layers; the biases are zero-mean and small; the linear weights are non-negative,
    as the trained ones are."""
    rs = np.random.RandomState(seed)
    vgg, lin, cin = {}, {}, 3
    for convs, c in zip(STAGE_CONVS, STAGE_CHANNELS):
        for n in convs:
            w = rs.standard_normal((c, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))
            vgg[f"features.{n}.weight"] = torch.from_numpy(w.astype(np.float32))
            vgg[f"features.{n}.bias"] = torch.from_numpy((0.05 * rs.standard_normal(c)).astype(np.float32))
            cin = c
    for k, c in enumerate(STAGE_CHANNELS):
        lin[f"lin{k}.model.1.weight"] = torch.from_numpy(rs.uniform(0.0, 1.0, (1, c, 1, 1)).astype(np.float32))
    return vgg, lin


def weight_checksums(vgg, lin):
    """(names, (n, 2) float64): every tensor's sum and sum of squares in fp64."""
    names = sorted(vgg) + sorted(lin)
    sums = [[float(t.double().sum()), float((t.double() ** 2).sum())] for t in [{**vgg, **lin}[n] for n in names]]
    return names, np.array(sums, np.float64)


def z_score(x: torch.Tensor) -> torch.Tensor:
    """(3, H, W) -> (1, 3, H, W); the constants are the fp32 ones in x's dtype (a module cast to
    fp64 keeps the fp32 buffers' values)."""
    mean = torch.tensor(MEAN, dtype=torch.float32, device=x.device).to(x.dtype)[None, :, None, None]
    std = torch.tensor(STD, dtype=torch.float32, device=x.device).to(x.dtype)[None, :, None, None]
    return (x - mean) / std


def masked_inputs(image, gt, alpha=None):
    """The two tensors the reference hands to lpips(): clamp(.) * alpha (render_hierarchy_final.py:
    144-145, 259-262)."""
    a = 1.0 if alpha is None else alpha.reshape(1, *alpha.shape[-2:])
    return image.clamp(0.0, 1.0) * a, gt.clamp(0.0, 1.0) * a


def trunk(x: torch.Tensor, vgg) -> list:
    """The five ReLU'd tap activations of one z-scored (1, 3, H, W) image."""
    out = []
    for k, convs in enumerate(STAGE_CONVS):
        if k:
            x = F.max_pool2d(x, 2, 2)
        for n in convs:
            w, b = vgg[f"features.{n}.weight"], vgg[f"features.{n}.bias"]
            x = F.relu(F.conv2d(x, w.to(x), b.to(x), padding=1))
        out.append(x)
    return out


def normalize_activation(x, eps=1e-10):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def nearest_index(n_out: int, n_in: int) -> np.ndarray:
    """The source index F.interpolate(mode='nearest') reads for each output index: fp32 throughout,
    scale = (float)n_in / n_out, src = min((int)floorf(i * scale), n_in - 1)."""
    scale = np.float32(n_in) / np.float32(n_out)
    src = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, n_in - 1)


def integer_index(n_out: int, n_in: int) -> np.ndarray:
    """The integer rule i * n_in // n_out, which is NOT torch's (see nearest_index)."""
    return np.arange(n_out, dtype=np.int64) * n_in // n_out


def resize_mask(mask: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """(H, W) -> (h, w) by the nearest rule, as float32 (the reference resizes mask.float())."""
    H, W = mask.shape
    r = torch.from_numpy(nearest_index(h, H)).to(mask.device)
    c = torch.from_numpy(nearest_index(w, W)).to(mask.device)
    return mask[r][:, c].float()


def stage_value(fx, fy, lin_w, mask=None):
    """One stage's term from the two ReLU'd feature maps (1, C, h, w): a 0-dim tensor."""
    d = (normalize_activation(fx) - normalize_activation(fy)) ** 2
    wd = F.conv2d(d, lin_w.to(d))
    if mask is None:
        return wd.mean((2, 3), True).reshape(())
    m = resize_mask(mask, wd.shape[2], wd.shape[3])[None, None]
    s = torch.sum(wd * m, dim=(2, 3), keepdim=True)
    area = torch.clamp(torch.sum(m, dim=(2, 3), keepdim=True), min=1e-8)
    return (s / area).reshape(())


def lin_weights(lin) -> list:
    return [lin[f"lin{k}.model.1.weight"] for k in range(len(STAGE_CHANNELS))]


def features(image, gt, alpha, vgg, dtype, device="cpu"):
    """The tap activations of both images, each run through the trunk on its own as the reference does."""
    x, y = masked_inputs(image.to(device=device, dtype=dtype), gt.to(device=device, dtype=dtype),
                         None if alpha is None else alpha.to(device=device, dtype=dtype))
    with torch.no_grad():
        return trunk(z_score(x), vgg), trunk(z_score(y), vgg)


def rows_from_features(fx, fy, lin, masks) -> torch.Tensor:
    """(5, 1 + len(masks)) in the features' dtype: every stage's term of the whole image (column 0)
    and of each (H, W) mask; the head is evaluated once per column."""
    with torch.no_grad():
        cols = [None] + [m.to(fx[0].device) for m in masks]
        return torch.stack([torch.stack([stage_value(a, b, w, m) for m in cols])
                            for a, b, w in zip(fx, fy, lin_weights(lin))])


def lpips_rows(image, gt, alpha, masks, weights, dtype=torch.float64, device="cpu") -> torch.Tensor:
    """(5, 1 + len(masks)) stage terms; .sum(0) is LPIPS per row."""
    vgg, lin = weights
    fx, fy = features(image, gt, alpha, vgg, dtype, device)
    return rows_from_features(fx, fy, lin, masks)


def lpips_call(x, y, weights, mask=None) -> torch.Tensor:
    """One call in the reference's structure: both trunks, then the head, for one row.  x, y: the
    masked inputs (3, H, W)."""
    vgg, lin = weights
    with torch.no_grad():
        fx, fy = trunk(z_score(x), vgg), trunk(z_score(y), vgg)
        return sum(stage_value(a, b, w, mask) for a, b, w in zip(fx, fy, lin_weights(lin)))


def masks_of_bits(bits: torch.Tensor, n: int) -> list:
    return [((bits.to(torch.int32) >> r) & 1).bool() for r in range(n)]
