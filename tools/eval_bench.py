"""Cost of the evaluation metrics of one frame on one GPU: the fused pass
(gs_train.evaluate.Evaluator.add: gsr_eval_frame + gsr_eval_accumulate) against the same metrics
composed from torch ops on the same device (tests/eval_ref.py frame_table in fp32 followed by its
accumulate on the device table), at 1920x1080 with R = 3 regions (the depth ranges) and R = 9 (the
depth ranges and six segmentation categories).

Seeded inputs: a smooth random image and a noisy copy, an alpha mask with a 10% hole, inverse depths
in [0, 0.4) varying smoothly so the depth ranges are contiguous areas, and a segmentation image of
rectangular patches in the six category colours and one unlabelled colour.  The region planes are
built before the timed window on both sides.  Device events around one call, a warm-up of both sides
at each R, then the two sides alternating; the torch side includes the `sum() == 0` host reads its
region loop makes, as the reference's loop does.  Reports the median and the spread (min .. max) per
side, and each side's largest error against the same composition in fp64 (computed once, untimed).

    python tools/eval_bench.py [--height 1080] [--width 1920] [--reps 15] [--out profiles/eval_bench.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "street-sparse-3dgs_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def smooth(g, shape, H, W, cells=12):
    """A smooth random field in [0, 1): bilinear upsampling of a coarse random grid."""
    coarse = torch.rand((1, shape, cells, cells * W // H + 1), generator=g)
    return F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)[0].clamp(0, 0.999999)


def inputs(H, W, dev):
    from gs_train.evaluate import CATEGORY_COLORS
    g = torch.Generator().manual_seed(17)
    img = smooth(g, 3, H, W, 40) * 1.1 - 0.05
    gt = img + 0.05 * torch.randn((3, H, W), generator=g)
    alpha = torch.ones((1, H, W))
    alpha[:, : H // 5, : W // 2] = 0.0
    gt_invd = smooth(g, 1, H, W, 6) * 0.4
    invd = gt_invd + 0.01 * torch.randn((1, H, W), generator=g)
    table = torch.tensor(list(CATEGORY_COLORS.values()) + [(0, 0, 0)], dtype=torch.uint8)
    patches = torch.randint(0, len(table), (1, 1, 9, 16), generator=g).float()
    label = F.interpolate(patches, size=(H, W), mode="nearest")[0, 0].long()
    seg = table[label].permute(2, 0, 1).contiguous()
    return [t.to(dev) for t in (img, gt, alpha, invd, gt_invd, seg)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "eval_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs a ROCm GPU: nothing is measured without one")
    import eval_ref
    from gs_train.evaluate import CATEGORY_COLORS, DEPTH_RANGES, Evaluator, category_bits, depth_range_bits
    dev = torch.device("cuda:0")
    H, W = a.height, a.width
    img, gt, alpha, invd, gt_invd, seg = inputs(H, W, dev)
    lines = [f"eval_bench: {torch.cuda.get_device_name(0)}, {W}x{H}, {a.reps} alternating runs after {a.warmup} "
             f"warm-up runs, ms per frame (median, min .. max)"]
    for R in (3, 9):
        bits = depth_range_bits(gt_invd, DEPTH_RANGES)
        if R == 9:
            category_bits(seg, tuple(CATEGORY_COLORS.values()), bits, shift=3)
        masks = eval_ref.masks_of_bits(bits, R)
        share = [float(m.float().mean()) for m in masks]
        ev = Evaluator(categories=R == 9)
        totals = torch.zeros((1 + R, 6), dtype=torch.float64, device=dev)

        def fused():
            return ev.add(img, gt, alpha, invd, gt_invd, bits)

        def composed():
            table = eval_ref.frame_table(img, gt, alpha, invd, gt_invd, masks, dtype=torch.float32)
            use = ((table[:, 5] != 0) & (table[:, 4] != 0)).to(torch.float64).unsqueeze(1)
            w = table[:, 4:5]
            totals.add_(use * torch.cat([w * table[:, :4], w, torch.ones_like(w)], 1))
            return table

        for _ in range(a.warmup):
            fused()
            composed()
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(a.reps):
            t, x = timed(fused)
            tf.append(t)
            t, y = timed(composed)
            tc.append(t)
        ref = eval_ref.frame_table(img, gt, alpha, invd, gt_invd, masks, dtype=torch.float64)  # untimed yardstick
        err = lambda t: " ".join(f"{d:.2e}" for d in (t[:, :4] - ref[:, :4]).abs().max(0).values.tolist())
        fmt = lambda v: f"{statistics.median(v):8.3f}  ({min(v):.3f} .. {max(v):.3f})"
        lines += [f"R = {R}  (region shares of the frame: " + " ".join(f"{s:.2f}" for s in share) + ")",
                  f"  fused Evaluator.add    {fmt(tf)}",
                  f"  torch composition      {fmt(tc)}",
                  f"  ratio of medians       {statistics.median(tc) / statistics.median(tf):8.1f}x",
                  "  largest error against the torch composition in fp64 (psnr dB, ssim, imae, irmse):",
                  f"    fused                {err(x)}",
                  f"    torch in fp32        {err(y)}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
