"""Evaluation metrics on the device: PSNR, SSIM, iMAE and iRMSE of a rendered frame, for the whole
image and per region (depth ranges, segmentation categories), fused into one gfx950 pass per frame
(csrc/eval.hip, include/gsr_eval.h), and their pixel-weighted running sums over a test set.

Replaces the per-frame metric loop of render_hierarchy_final.py:259-390 (compute_metrics,
compute_depth_metrics, get_depth_range_mask, the category colour match) and its report
(:390-438).  A region is one bit of a 16-bit plane; the frame is read once however many regions
there are, and a whole test set needs one device-to-host read, in Evaluator.result().

LPIPS is the caller's choice: Evaluator(lpips=LpipsModel...) (gs_train/lpips.py, with the caller's VGG
and LPIPS weights -- this package carries none) adds the reference's third image metric to every row,
from one trunk pass per frame, and the report lines are then the reference's field for field.
Without a model the tables, the result keys and the report lines carry no LPIPS field.

One documented divergence: a region that has pixels in a frame but none where the alpha mask is
positive has weight 0 and is left out of the sums (the reference would add inf * 0 = NaN).
"""
from __future__ import annotations

import ctypes
import math

import torch

from ._native import check, lib, ptr, require_gpu, stream

MAX_REGIONS = 16
FRAME_COLS = ("psnr", "ssim", "imae", "irmse", "weight", "evaluated", "mask_pixels", "valid_windows")

# render_hierarchy_final.py:31-35: (lo, hi) in metres, lo <= depth < hi
DEPTH_RANGES = ((0.0, 5.0), (5.0, 20.0), (20.0, math.inf))
DEPTH_RANGE_NAMES = ("near", "medium", "far")
# render_hierarchy_final.py:21-28: the segmentation images' category colours
CATEGORY_COLORS = {
    "sky": (0x87, 0xCE, 0xEB),
    "ground": (0x8B, 0x45, 0x13),
    "buildings": (0x69, 0x69, 0x69),
    "vehicles": (0xFF, 0x45, 0x00),
    "vegetation": (0x22, 0x8B, 0x22),
    "lamposts": (0xFF, 0xD7, 0x00),
}

_BITS_DTYPES = tuple(d for d in (torch.int16, getattr(torch, "uint16", None)) if d is not None)


def _check_bits(bits, shape, shift, n):
    if shift < 0 or n < 0 or shift + n > MAX_REGIONS:
        raise ValueError(f"bits {shift}..{shift + n - 1} do not fit a 16-bit plane")
    if bits is not None:
        if bits.dtype not in _BITS_DTYPES:
            raise ValueError(f"the bits plane must be 16-bit (torch.int16), got {bits.dtype}")
        if tuple(bits.shape) != tuple(shape) or not bits.is_contiguous():
            raise ValueError(f"the bits plane must be contiguous of shape {tuple(shape)}, got {tuple(bits.shape)}")


def depth_range_bits(gt_invdepth: torch.Tensor, ranges=DEPTH_RANGES, bits: torch.Tensor | None = None,
                     shift: int = 0) -> torch.Tensor:
    """OR bit shift + k into the (H, W) plane `bits` (a new zero plane when None) where
    lo_k <= 1 / (gt_invdepth + 1e-6) < hi_k in fp32 (get_depth_range_mask,
    render_hierarchy_final.py:121-139)."""
    hw = gt_invdepth.shape[-2:]
    if gt_invdepth.numel() != hw[0] * hw[1]:
        raise ValueError(f"expected an (H, W) or (1, H, W) inverse depth map, got {tuple(gt_invdepth.shape)}")
    ranges = tuple(ranges)
    _check_bits(bits, hw, shift, len(ranges))
    require_gpu(gt_invdepth, bits)
    d = gt_invdepth.detach().float().contiguous()
    if bits is None:
        bits = torch.zeros(hw, dtype=torch.int16, device=d.device)
    lo = (ctypes.c_float * max(1, len(ranges)))(*[float(r[0]) for r in ranges])
    hi = (ctypes.c_float * max(1, len(ranges)))(*[float(r[1]) for r in ranges])
    check(lib().gsr_eval_depth_range_bits(ptr(d), d.numel(), len(ranges), lo, hi, shift, ptr(bits), stream(d.device)),
          "gsr_eval_depth_range_bits")
    return bits


def category_bits(seg_rgb_u8: torch.Tensor, colors=tuple(CATEGORY_COLORS.values()), bits: torch.Tensor | None = None,
                  shift: int = 0) -> torch.Tensor:
    """OR bit shift + k into `bits` where the three channels of the uint8 (3, H, W) segmentation
    image (an RGBA image's first three) equal colour k (render_hierarchy_final.py:353-358)."""
    if seg_rgb_u8.dim() != 3 or seg_rgb_u8.shape[0] not in (3, 4) or seg_rgb_u8.dtype != torch.uint8:
        raise ValueError("expected a uint8 (3, H, W) or (4, H, W) segmentation image")
    colors = [tuple(int(v) for v in c) for c in colors]
    if any(len(c) != 3 or min(c) < 0 or max(c) > 255 for c in colors):
        raise ValueError("colours are (r, g, b) triples of 0..255")
    hw = seg_rgb_u8.shape[-2:]
    _check_bits(bits, hw, shift, len(colors))
    require_gpu(seg_rgb_u8, bits)
    seg = seg_rgb_u8[:3].contiguous()
    if bits is None:
        bits = torch.zeros(hw, dtype=torch.int16, device=seg.device)
    flat = (ctypes.c_uint8 * max(1, 3 * len(colors)))(*[v for c in colors for v in c])
    check(lib().gsr_eval_color_bits(ptr(seg), hw[0] * hw[1], len(colors), flat, shift, ptr(bits), stream(seg.device)),
          "gsr_eval_color_bits")
    return bits


def _plane(t, hw, what):
    if t is None:
        return None
    if t.dim() not in (2, 3) or tuple(t.shape[-2:]) != tuple(hw) or t.numel() != hw[0] * hw[1]:
        raise ValueError(f"{what} must be (H, W) or (1, H, W) = {tuple(hw)}, got {tuple(t.shape)}")
    return t


def frame_metrics(image: torch.Tensor, gt: torch.Tensor, alpha_mask: torch.Tensor | None = None,
                  invdepth: torch.Tensor | None = None, gt_invdepth: torch.Tensor | None = None,
                  region_bits: torch.Tensor | None = None, n_regions: int = 0) -> torch.Tensor:
    """The (1 + n_regions, 8) float64 device table of one frame (columns FRAME_COLS; row 0 the whole
    image, row 1 + r the region of bit r).  image, gt: (3, H, W), unclamped; alpha_mask: (H, W) or
    (1, H, W) or None (all ones); invdepth and gt_invdepth go together (None: imae = irmse = 0).
    No host sync."""
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"expected a (3, H, W) image, got {tuple(image.shape)}")
    if image.shape != gt.shape:
        raise ValueError(f"image shapes differ: {tuple(image.shape)} vs {tuple(gt.shape)}")
    hw = tuple(image.shape[-2:])
    _plane(alpha_mask, hw, "alpha_mask")
    if (invdepth is None) != (gt_invdepth is None):
        raise ValueError("invdepth and gt_invdepth go together")
    _plane(invdepth, hw, "invdepth")
    _plane(gt_invdepth, hw, "gt_invdepth")
    n_regions = int(n_regions)
    if n_regions < 0 or n_regions > MAX_REGIONS:
        raise ValueError(f"n_regions must be 0..{MAX_REGIONS}, got {n_regions}")
    if n_regions > 0 and region_bits is None:
        raise ValueError("regions need a region_bits plane")
    _check_bits(region_bits, hw, 0, n_regions)
    require_gpu(image, gt, alpha_mask, invdepth, gt_invdepth, region_bits)

    f = lambda t: None if t is None else t.detach().float().contiguous()
    image, gt, alpha_mask, invdepth, gt_invdepth = f(image), f(gt), f(alpha_mask), f(invdepth), f(gt_invdepth)
    H, W = hw
    L = lib()
    dev = image.device
    scratch = torch.empty(max(1, L.gsr_eval_frame_scratch_bytes(H, W, n_regions)), dtype=torch.uint8, device=dev)
    frame = torch.empty((1 + n_regions, len(FRAME_COLS)), dtype=torch.float64, device=dev)
    check(L.gsr_eval_frame(ptr(image), ptr(gt), ptr(alpha_mask), ptr(invdepth), ptr(gt_invdepth),
                           ptr(region_bits) if n_regions else ctypes.c_void_p(0), n_regions, H, W, ptr(scratch),
                           ptr(frame), stream(dev)), "gsr_eval_frame")
    return frame


def _get(view, name):
    return view.get(name) if isinstance(view, dict) else getattr(view, name, None)


class Evaluator:
    """Pixel-weighted running metric sums of a test set, kept on the device.

    region_names: one name per region bit, in bit order.  None: the three depth ranges
    (depth_near, depth_medium, depth_far), followed by the six categories when categories=True --
    the layout add_view builds.  lpips: a gs_train.lpips.LpipsModel, or None (no LPIPS column)."""

    def __init__(self, region_names=None, categories: bool = False, lpips=None):
        self._standard = region_names is None
        if region_names is None:
            region_names = ["depth_" + n for n in DEPTH_RANGE_NAMES] + (list(CATEGORY_COLORS) if categories else [])
        self.region_names = [str(n) for n in region_names]
        if len(self.region_names) > MAX_REGIONS:
            raise ValueError(f"at most {MAX_REGIONS} regions, got {len(self.region_names)}")
        if len(set(self.region_names) | {"whole_image"}) != len(self.region_names) + 1:
            raise ValueError("region names must be distinct and not 'whole_image'")
        self.categories = bool(categories) and self._standard
        self.totals = None  # (1 + R, 6) float64 on the device of the first frame
        self.lpips = lpips
        self.lpips_totals = None  # (1 + R, 2) float64 beside it: sum w lpips, sum w

    @property
    def n_regions(self):
        return len(self.region_names)

    def add(self, image, gt, alpha_mask=None, invdepth=None, gt_invdepth=None, region_bits=None) -> torch.Tensor:
        """Add one frame; returns its frame_metrics table.  No host sync."""
        frame = frame_metrics(image, gt, alpha_mask, invdepth, gt_invdepth, region_bits, self.n_regions)
        if self.totals is None:
            self.totals = torch.zeros((1 + self.n_regions, 6), dtype=torch.float64, device=frame.device)
        check(lib().gsr_eval_accumulate(ptr(frame), 1 + self.n_regions, ptr(self.totals), stream(frame.device)),
              "gsr_eval_accumulate")
        if self.lpips is not None:
            from .lpips import accumulate
            rows = self.lpips.frame(image, gt, alpha_mask, region_bits, self.n_regions)
            if self.lpips_totals is None:
                self.lpips_totals = torch.zeros((1 + self.n_regions, 2), dtype=torch.float64, device=frame.device)
            accumulate(rows, frame, self.lpips_totals)
        return frame

    def add_view(self, render_pkg, view, half: bool = False) -> torch.Tensor:
        """Add the frame of one test view.  render_pkg: a dict with "render" (3, H, W) and "depth"
        (the inverse depth, (1, H, W)) from any of the render paths.  view: an object or dict with
        original_image, alpha_mask (or None), invdepthmap and, for the categories, segmentation (a
        uint8 (3 or 4, H, W) image, or None: the frame's category rows are then not evaluated).
        half=True: the train_test_exp crop to the right half (render_hierarchy_final.py:265-268),
        applied to every map."""
        if not self._standard:
            raise ValueError("add_view builds the standard regions: construct Evaluator() without region_names")
        crop = (lambda t: t if t is None else t[..., t.shape[-1] // 2:]) if half else (lambda t: t)
        image, depth = crop(render_pkg["render"]), crop(render_pkg["depth"])
        gt, alpha = crop(_get(view, "original_image")), crop(_get(view, "alpha_mask"))
        gt_depth, seg = crop(_get(view, "invdepthmap")), crop(_get(view, "segmentation"))
        if gt_depth is None:
            raise ValueError("the view has no invdepthmap: the depth ranges need it")
        gt_depth = gt_depth.to(image.device)
        bits = depth_range_bits(gt_depth, DEPTH_RANGES)
        if self.categories and seg is not None:
            category_bits(seg.to(image.device), tuple(CATEGORY_COLORS.values()), bits, shift=len(DEPTH_RANGES))
        return self.add(image, gt.to(image.device), None if alpha is None else alpha.to(image.device), depth, gt_depth,
                        bits)

    def result(self, totals=None, lpips_totals=None) -> dict:
        """{name: {psnr, ssim, imae, irmse, pixel_count, image_count}}: each metric's weighted sum
        divided by the summed weight (render_hierarchy_final.py:398-435), None where nothing was
        evaluated; with a model also lpips, after ssim.  The one device-to-host read (two with a
        model)."""
        t = self.totals if totals is None else totals
        rows = [[0.0] * 6] * (1 + self.n_regions) if t is None else torch.as_tensor(t).cpu().tolist()
        lp = None
        if self.lpips is not None:
            lt = self.lpips_totals if lpips_totals is None else lpips_totals
            lp = [[0.0] * 2] * (1 + self.n_regions) if lt is None else torch.as_tensor(lt).cpu().tolist()
        out = {}
        for k, (name, r) in enumerate(zip(["whole_image"] + self.region_names, rows)):
            n = int(r[5])
            m = [v / r[4] if n > 0 else None for v in r[:4]]
            out[name] = {"psnr": m[0], "ssim": m[1]}
            if lp is not None:
                out[name]["lpips"] = lp[k][0] / r[4] if n > 0 else None
            out[name].update({"imae": m[2], "irmse": m[3], "pixel_count": int(r[4]), "image_count": n})
        return out

    def format(self, totals=None, lpips_totals=None) -> list:
        """The reference's report lines (render_hierarchy_final.py:403-437); the LPIPS field is there
        with a model and absent without."""
        res = self.result(totals, lpips_totals)

        def metrics(r):
            lp = f"LPIPS: {r['lpips']:.5f} " if "lpips" in r else ""
            return (f"PSNR: {r['psnr']:.5f} SSIM: {r['ssim']:.5f} {lp}iMAE: {r['imae']:.5f} iRMSE: {r['irmse']:.5f} "
                    f"(pixel-weighted and evaluated on {r['image_count']} ")

        lines = []
        r = res["whole_image"]
        if r["image_count"] > 0:
            lines.append("Whole Image: " + metrics(r) + "images)")
        depth = {"depth_" + n: (n, lo, hi) for n, (lo, hi) in zip(DEPTH_RANGE_NAMES, DEPTH_RANGES)}
        names = self.region_names
        if self._standard:
            lines += ["", "Depth-Stratified Results:"]
            for key in names[:len(DEPTH_RANGES)]:
                n, lo, hi = depth[key]
                label = f"  {n.capitalize()} ({lo}m+)" if hi == math.inf else f"  {n.capitalize()} ({lo}-{hi}m)"
                r = res[key]
                lines.append(f"{label}: " + (metrics(r) + "instances)" if r["image_count"] > 0
                                             else "No valid pixels found in this depth range."))
            names = names[len(DEPTH_RANGES):]
            if names:
                lines += ["", "Category-Specific Results:"]
        for key in names:
            r = res[key]
            kind = "Category" if self._standard else "Region"
            lines.append(f"  {kind} '{key}' : " + (metrics(r) + "images)" if r["image_count"] > 0
                                                   else "Not found or no valid overlap in any evaluated image."))
        return lines
