"""LPIPS (VGG16, v0.1) of a rendered frame, for the whole image and per region, with one trunk pass per
frame (csrc/lpips.hip, include/gsr_lpips.h).

Replaces the lpips(...) calls of render_hierarchy_final.py:142-157 (lpipsPyTorch/modules/lpips.py,
networks.py, utils.py): the reference runs the VGG16 trunk on both images once for the whole image
and once more per depth range and per category, and applies the region's mask only in the last step.
The trunk's inputs are the same for every row, so LpipsModel.frame runs it once on a batch of two;
after each of the five stages one kernel reads the stage's feature maps once and leaves the stage's
term of every row, and the pooled input of the next stage.

The weights are the caller's: the 13 convolutions of torchvision's VGG16 (IMAGENET1K_V1) and the five
linear layers of LPIPS v0.1 "vgg", as state dicts or as files read with weights_only=True.  This
package carries none and fetches none.

The 13 convolutions run in torch (LpipsModel._convs: F.conv2d, fp32, no_grad); everything around
them -- the input batch, the ReLU in front of every tap, the channel normalisation, the weighted
squared difference, the nearest-neighbour mask resize, the masked means and the max pooling -- is
native.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn.functional as F

from ._native import check, lib, ptr, require_gpu, stream

MAX_REGIONS = 16
# torchvision's vgg16().features: the index of every convolution, grouped by stage; a tap follows the
# ReLU of each stage's last convolution (target_layers = [4, 9, 16, 23, 30] counted from 1,
# lpipsPyTorch/modules/networks.py:57-59, 93) and a 2x2 max pool separates the stages
STAGE_CONVS = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
STAGE_CHANNELS = (64, 128, 256, 512, 512)
MIN_SIZE = 16  # four floor-mode poolings leave at least one pixel for stage five

_BITS_DTYPES = tuple(d for d in (torch.int16, getattr(torch, "uint16", None)) if d is not None)


def _conv_shapes():
    cin, out = 3, []
    for convs, c in zip(STAGE_CONVS, STAGE_CHANNELS):
        for n in convs:
            out.append((n, c, cin))
            cin = c
    return out


def _lookup(sd, names, what):
    for n in names:
        if n in sd:
            return sd[n]
    raise KeyError(f"{what}: none of {names} in the state dict")


class LpipsModel:
    """The weights of LPIPS-VGG on one device: 13 (weight, bias) pairs and five linear vectors."""

    def __init__(self, convs, lins):
        self.convs = convs  # [[(weight, bias), ...] per stage]
        self.lins = lins    # [(C,) per stage]
        self.device = lins[0].device
        self.miopen = False  # see _convs

    @classmethod
    def from_state_dicts(cls, vgg_features, lin, device="cuda") -> "LpipsModel":
        """vgg_features: the convolutions as `features.N.weight` / `features.N.bias` (torchvision's
        vgg16 state dict; the classifier's entries are ignored) or `N.weight` / `N.bias` (its
        .features).  lin: the linear layers as `linK.model.1.weight` (the LPIPS weight file, K = 0..4)
        or `K.1.weight` (the reference's renamed keys, modules/utils.py:22-28).  Shapes are checked."""
        dev = torch.device(device)
        f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
        shapes = iter(_conv_shapes())
        convs = []
        for stage in STAGE_CONVS:
            row = []
            for _ in stage:
                n, cout, cin = next(shapes)
                w = _lookup(vgg_features, (f"features.{n}.weight", f"{n}.weight"), f"convolution {n}")
                b = _lookup(vgg_features, (f"features.{n}.bias", f"{n}.bias"), f"convolution {n}")
                if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                    raise ValueError(f"convolution {n}: expected weight {(cout, cin, 3, 3)} and bias {(cout,)}, got "
                                     f"{tuple(w.shape)} and {tuple(b.shape)}")
                row.append((f(w), f(b)))
            convs.append(row)
        lins = []
        for k, c in enumerate(STAGE_CHANNELS):
            w = _lookup(lin, (f"lin{k}.model.1.weight", f"{k}.1.weight"), f"linear layer {k}")
            if tuple(w.shape) != (1, c, 1, 1):
                raise ValueError(f"linear layer {k}: expected weight {(1, c, 1, 1)}, got {tuple(w.shape)}")
            lins.append(f(w).reshape(c))
        return cls(convs, lins)

    @classmethod
    def load(cls, vgg_path, lin_path, device="cuda") -> "LpipsModel":
        """Read the two weight files (tensors only: weights_only=True)."""
        return cls.from_state_dicts(torch.load(vgg_path, map_location="cpu", weights_only=True),
                                    torch.load(lin_path, map_location="cpu", weights_only=True), device)

    def _convs(self, x: torch.Tensor, stage: int) -> torch.Tensor:
        """The stage's convolutions with bias and ReLU between them; the last one's output is left
        pre-ReLU for the tap.  The one place the trunk's GEMM work is done.  MIOpen is bypassed unless
        self.miopen is set: its first call per shape searches and compiles for seconds, and every
        frame size brings 13 new shapes."""
        with torch.backends.cudnn.flags(enabled=self.miopen):
            row = self.convs[stage]
            for k, (w, b) in enumerate(row):
                x = F.conv2d(x, w, b, padding=1)
                if k + 1 < len(row):
                    x = F.relu_(x)
        return x

    @torch.no_grad()
    def frame(self, image: torch.Tensor, gt: torch.Tensor, alpha_mask: torch.Tensor | None = None,
              region_bits: torch.Tensor | None = None, n_regions: int = 0) -> torch.Tensor:
        """The (1 + n_regions,) float64 device vector of one frame's LPIPS: row 0 the whole image,
        row 1 + r the region of bit r of the (H, W) 16-bit plane `region_bits` (an empty region's row
        is 0).  image, gt: (3, H, W), unclamped; alpha_mask: (H, W) or (1, H, W) or None (all ones).
        No host sync."""
        if image.dim() != 3 or image.shape[0] != 3:
            raise ValueError(f"expected a (3, H, W) image, got {tuple(image.shape)}")
        if image.shape != gt.shape:
            raise ValueError(f"image shapes differ: {tuple(image.shape)} vs {tuple(gt.shape)}")
        H, W = (int(v) for v in image.shape[-2:])
        if H < MIN_SIZE or W < MIN_SIZE:
            raise ValueError(f"LPIPS-VGG needs H, W >= {MIN_SIZE} (the fifth stage would be empty), got {(H, W)}")
        if alpha_mask is not None and (alpha_mask.dim() not in (2, 3) or tuple(alpha_mask.shape[-2:]) != (H, W)
                                       or alpha_mask.numel() != H * W):
            raise ValueError(f"alpha_mask must be (H, W) or (1, H, W) = {(H, W)}, got {tuple(alpha_mask.shape)}")
        n_regions = int(n_regions)
        if n_regions < 0 or n_regions > MAX_REGIONS:
            raise ValueError(f"n_regions must be 0..{MAX_REGIONS}, got {n_regions}")
        if n_regions > 0:
            if region_bits is None:
                raise ValueError("regions need a region_bits plane")
            if region_bits.dtype not in _BITS_DTYPES:
                raise ValueError(f"the bits plane must be 16-bit (torch.int16), got {region_bits.dtype}")
            if tuple(region_bits.shape) != (H, W) or not region_bits.is_contiguous():
                raise ValueError(f"the bits plane must be contiguous of shape {(H, W)}, got {tuple(region_bits.shape)}")
        require_gpu(image, gt, alpha_mask, region_bits if n_regions else None)
        if image.device != self.device:
            raise ValueError(f"the frame is on {image.device}, the model on {self.device}")

        f = lambda t: None if t is None else t.detach().float().contiguous()
        image, gt, alpha_mask = f(image), f(gt), f(alpha_mask)
        L, dev, st = lib(), image.device, stream(image.device)
        bits = ptr(region_bits) if n_regions else ctypes.c_void_p(0)
        x = torch.empty((2, 3, H, W), dtype=torch.float32, device=dev)
        check(L.gsr_lpips_prepare(ptr(image), ptr(gt), ptr(alpha_mask), H, W, ptr(x), st), "gsr_lpips_prepare")
        terms = torch.empty((len(STAGE_CONVS), 1 + n_regions), dtype=torch.float64, device=dev)
        for k, C in enumerate(STAGE_CHANNELS):
            feat = self._convs(x, k)
            h, w = (int(v) for v in feat.shape[-2:])
            last = k + 1 == len(STAGE_CHANNELS)
            x = None if last else torch.empty((2, C, h // 2, w // 2), dtype=torch.float32, device=dev)
            scratch = torch.empty(max(1, L.gsr_lpips_tap_scratch_bytes(h, w, n_regions)), dtype=torch.uint8, device=dev)
            check(L.gsr_lpips_tap(ptr(feat), ptr(self.lins[k]), C, h, w, bits, n_regions, H, W,
                                  ctypes.c_void_p(0) if last else ptr(x), ptr(scratch), ptr(terms[k]), st),
                  "gsr_lpips_tap")
        # stage by stage: torch's sum(0) picks its order by the shape, and a row must not depend on
        # how many regions ride along
        return (((terms[0] + terms[1]) + terms[2]) + terms[3]) + terms[4]


def accumulate(lpips_rows: torch.Tensor, frame: torch.Tensor, totals: torch.Tensor) -> None:
    """totals (n_rows, 2) += (weight * lpips, weight) for the rows gsr_eval_accumulate counts in the
    frame_metrics table `frame` of the same frame (evaluated, weight > 0)."""
    n = int(lpips_rows.numel())
    if tuple(frame.shape) != (n, 8) or tuple(totals.shape) != (n, 2):
        raise ValueError(f"expected a ({n}, 8) frame table and ({n}, 2) totals, got {tuple(frame.shape)} and "
                         f"{tuple(totals.shape)}")
    for t in (lpips_rows, frame, totals):
        if t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("lpips rows, frame table and totals are contiguous float64 tensors")
    require_gpu(lpips_rows, frame, totals)
    check(lib().gsr_lpips_accumulate(ptr(lpips_rows), ptr(frame), n, ptr(totals), stream(totals.device)),
          "gsr_lpips_accumulate")
