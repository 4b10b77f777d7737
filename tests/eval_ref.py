"""The evaluation metrics of include/gsr_eval.h restated with torch ops, for the tests and for
tools/eval_bench.py: fp64 on the CPU as the yardstick of the kernels, or any dtype on any device (the
"same metrics composed from torch ops" of the measurement).

Written from the formulas (utils/image_utils.py:17-36 psnr / psnr_masked, utils/loss_utils.py:23-61
ssim, :85-153 ssim_masked, render_hierarchy_final.py:121-139 get_depth_range_mask, :159-173
compute_depth_metrics, :285-313 the weights); tests/golden/eval.npz holds what the reference's own
functions return.
"""
from __future__ import annotations

from math import exp

import torch
import torch.nn.functional as F

COLS = ("psnr", "ssim", "imae", "irmse", "weight", "evaluated", "mask_pixels", "valid_windows")
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window(dtype=torch.float64, device="cpu"):
    """The (3, 1, 11, 11) depthwise window: fp32 taps normalised by their fp32 sum, their fp32 outer
    product, then cast (utils/loss_utils.py:23-31, window.type_as(img))."""
    g = torch.tensor([exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).float().expand(3, 1, 11, 11).contiguous().to(device=device, dtype=dtype)


def depth_range_mask(gt_invdepth: torch.Tensor, lo: float, hi: float) -> torch.Tensor:
    """lo <= 1 / (gt_invdepth + 1e-6) < hi in the input's precision (fp32 in the reference)."""
    depth = 1.0 / (gt_invdepth + 1e-6)
    return (depth >= lo) & (depth < hi)


def color_mask(seg_rgb_u8: torch.Tensor, color) -> torch.Tensor:
    return (seg_rgb_u8[0] == color[0]) & (seg_rgb_u8[1] == color[1]) & (seg_rgb_u8[2] == color[2])


def masks_of_bits(bits: torch.Tensor, n: int):
    b = bits.to(torch.int32) & 0xFFFF
    return [((b >> r) & 1).bool() for r in range(n)]


def masked_ssim_terms(x, y, m, win):
    """(w, valid, numerator, denominator) of ssim_masked for (3, H, W) x, y and a (1, H, W) 0/1 mask."""
    conv = lambda t: F.conv2d(t[None], win, padding=5, groups=3)[0]
    m3 = m.expand_as(x)
    xm, ym = x * m3, y * m3
    w = conv(m3.contiguous())
    valid = w > 1e-6
    ws = torch.where(valid, w, torch.ones_like(w))
    zero = torch.zeros_like(w)
    mu1 = torch.where(valid, conv(xm) / ws, zero)
    mu2 = torch.where(valid, conv(ym) / ws, zero)
    s1 = torch.where(valid, conv(xm * xm) / ws - mu1 * mu1, zero)
    s2 = torch.where(valid, conv(ym * ym) / ws - mu2 * mu2, zero)
    s12 = torch.where(valid, conv(xm * ym) / ws - mu1 * mu2, zero)
    num = (2 * mu1 * mu2 + C1) * (2 * s12 + C2)
    den = (mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2)
    return w, valid, num, den


def frame_table(image, gt, alpha=None, invdepth=None, gt_invdepth=None, masks=(), dtype=torch.float64):
    """The (1 + len(masks), 8) table of gsr_eval_frame (columns COLS), computed in `dtype` on the
    inputs' device and returned as float64.  image, gt: (3, H, W) unclamped; alpha, invdepth,
    gt_invdepth: (H, W) or (1, H, W) or None; masks: (H, W) boolean or 0/1 planes."""
    dev = image.device
    H, W = image.shape[-2:]
    c = lambda t: t.to(dtype)
    a = torch.ones((1, H, W), dtype=dtype, device=dev) if alpha is None else c(alpha).reshape(1, H, W)
    x = c(image.clamp(0.0, 1.0)) * a
    y = c(gt.clamp(0.0, 1.0)) * a
    win = window(dtype, dev)
    conv = lambda t: F.conv2d(t[None], win, padding=5, groups=3)[0]
    zero = torch.zeros((), dtype=dtype, device=dev)
    sq = (x - y) ** 2
    if invdepth is not None:
        dd = c(invdepth).reshape(1, H, W) - c(gt_invdepth).reshape(1, H, W)

    def depth_metrics(mask):
        if invdepth is None:
            return zero, zero
        n = mask.sum()
        ok = n > 0
        return (torch.where(ok, (dd.abs() * mask).sum() / n, zero),
                torch.where(ok, torch.sqrt((dd * dd * mask).sum() / n), zero))

    def row(*v):
        return torch.stack([torch.as_tensor(t, dtype=torch.float64, device=dev) for t in v])

    rows = []
    psnr = (20 * torch.log10(1.0 / torch.sqrt(sq.reshape(3, -1).mean(1)))).mean()
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    ssim = (((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))).mean()
    imae, irmse = depth_metrics(a)
    rows.append(row(psnr, ssim, imae, irmse, H * W, 1, H * W, H * W))
    for m in masks:
        m = c(m).reshape(1, H, W)
        n = m.sum()
        if n == 0:
            rows.append(torch.zeros(8, dtype=torch.float64, device=dev))
            continue
        psnr = (20 * torch.log10(1.0 / torch.sqrt((sq * m).reshape(3, -1).sum(1) / n))).mean()
        w, valid, num, den = masked_ssim_terms(x, y, m, win)
        keep = valid & (den > 1e-10)
        smap = torch.where(keep, num / torch.where(keep, den, torch.ones_like(den)), torch.zeros_like(den)) * m
        mv = m * valid.to(dtype)
        ssim = smap.sum() / mv.sum().clamp(min=1)
        am = a * m
        imae, irmse = depth_metrics(am)
        rows.append(row(psnr, ssim, imae, irmse, (am > 0).sum(), 1, n, mv[0].sum()))
    return torch.stack(rows)


def accumulate(totals: torch.Tensor, frame: torch.Tensor) -> torch.Tensor:
    """gsr_eval_accumulate on the host in fp64: totals (rows, 6) += the frame's rows."""
    totals = totals.clone()
    for r in range(frame.shape[0]):
        w = frame[r, 4]
        if frame[r, 5] == 0 or w == 0:
            continue
        totals[r, :4] += w * frame[r, :4]
        totals[r, 4] += w
        totals[r, 5] += 1
    return totals


def tolerances(g) -> dict:
    """{kind: (psnr dB, ssim, imae relative, irmse relative)}: max(floor, 4 D) with the D the
    fixture records per kind of region ("single": one-pixel regions, "other": the rest)."""
    floors = (1e-5, 2e-6, 1e-6, 1e-6)
    return {kind: tuple(max(f, 4.0 * float(d)) for f, d in zip(floors, g["D_" + kind])) for kind in ("single", "other")}


def check_rows(got, want, kinds, tol, what=""):
    """Assert the metric columns of `got` (rows, >= 4) against `want` under tolerances()."""
    import math
    for r, kind in enumerate(kinds):
        t = tol[kind]
        for k, name in enumerate(COLS[:4]):
            a, b = float(got[r][k]), float(want[r][k])
            if math.isinf(b) or math.isinf(a):
                assert a == b, f"{what} row {r} {name}: {a} vs {b}"
                continue
            err = abs(a - b) / abs(b) if k >= 2 and b != 0 else abs(a - b)
            assert err <= t[k], f"{what} row {r} ({kind}) {name}: {a!r} vs {b!r}, error {err:.3e} > {t[k]:.3e}"
