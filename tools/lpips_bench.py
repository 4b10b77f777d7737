"""Cost of LPIPS of one frame on one GPU: the fused path (gs_train.lpips.LpipsModel.frame:
one trunk pass over a batch of two, gsr_lpips_prepare and five gsr_lpips_tap calls) against the same
metric in the reference's call structure (tests/lpips_ref.py lpips_call in fp32 on the same device: one
full call -- both trunks and the head -- for the whole image and one more per region), at 1536x1536
with R = 3 regions (the depth ranges) and R = 9 (the depth ranges and six categories).

Seeded inputs: a smooth random image and a noisy copy, an alpha mask with a hole, and region planes of
smooth contiguous areas.  The weights are tests/lpips_ref.make_weights(0) -- VGG16-shaped random
tensors, not the trained ones -- so the times are those of the real network and the values are not.
Both sides run their convolutions through the same torch backend (MIOpen bypassed unless --miopen).
Device events around one call, a warm-up of both sides at each R, then the two sides alternating.
The fused side is split with events around its convolution calls: trunk, and everything else
(prepare, taps, finalize, the sum over the stages).  Reports the median and the spread (min .. max).

    python tools/lpips_bench.py [--size 1536] [--reps 15] [--miopen] [--out profiles/lpips_bench.txt]
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
    g = torch.Generator().manual_seed(19)
    img = smooth(g, 3, H, W, 40) * 1.1 - 0.05
    gt = img + 0.05 * torch.randn((3, H, W), generator=g)
    alpha = torch.ones((H, W))
    alpha[: H // 5, : W // 2] = 0.0
    depth = smooth(g, 1, H, W, 6)[0]
    label = F.interpolate(torch.randint(0, 7, (1, 1, 9, 16), generator=g).float(), size=(H, W), mode="nearest")[0, 0]
    bits = torch.zeros((H, W), dtype=torch.int32)
    for r, (lo, hi) in enumerate(((0.0, 0.4), (0.4, 0.7), (0.7, 1.0))):
        bits |= ((depth >= lo) & (depth < hi)).int() << r
    for c in range(6):  # label 6: unlabelled
        bits |= (label == c).int() << (3 + c)
    return img.to(dev), gt.to(dev), alpha.to(dev), bits.to(torch.int16).to(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1536)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--miopen", action="store_true", help="run both sides' convolutions through MIOpen")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lpips_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench needs a ROCm GPU: nothing is measured without one")
    import lpips_ref
    from gs_train.lpips import LpipsModel
    dev = torch.device("cuda:0")
    H = W = a.size
    img, gt, alpha, bits = inputs(H, W, dev)
    weights = lpips_ref.make_weights(0)
    model = LpipsModel.from_state_dicts(*weights, device=dev)
    model.miopen = a.miopen
    dev_weights = tuple({k: v.to(dev) for k, v in d.items()} for d in weights)

    spans = []  # (start, end) events around the fused side's convolution calls
    convs = model._convs

    def timed_convs(x, stage):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = convs(x, stage)
        e.record()
        spans.append((s, e))
        return out

    model._convs = timed_convs
    lines = [f"lpips_bench: {torch.cuda.get_device_name(0)}, {W}x{H}, generated weights, convolutions through "
             f"{'MIOpen' if a.miopen else 'torch (MIOpen bypassed)'}, {a.reps} alternating runs after {a.warmup} "
             f"warm-up runs, ms per frame (median, min .. max)"]
    for R in (3, 9):
        masks = lpips_ref.masks_of_bits(bits, R)
        share = [float(m.float().mean()) for m in masks]

        def fused():
            return model.frame(img, gt, alpha, bits, R)

        def reference():
            with torch.backends.cudnn.flags(enabled=a.miopen):
                x, y = lpips_ref.masked_inputs(img, gt, alpha)
                return torch.stack([lpips_ref.lpips_call(x, y, dev_weights, m) for m in [None] + masks])

        for _ in range(a.warmup):
            fused()
            reference()
        torch.cuda.synchronize()
        tf, tt, tr = [], [], []
        for _ in range(a.reps):
            spans.clear()
            t, x = timed(fused)
            tf.append(t)
            tt.append(sum(s.elapsed_time(e) for s, e in spans))
            t, y = timed(reference)
            tr.append(t)
        rest = [f - t for f, t in zip(tf, tt)]
        fmt = lambda v: f"{statistics.median(v):9.3f}  ({min(v):.3f} .. {max(v):.3f})"
        lines += [f"R = {R}  (region shares of the frame: " + " ".join(f"{s:.2f}" for s in share) + ")",
                  f"  fused LpipsModel.frame       {fmt(tf)}",
                  f"    trunk (13 convolutions)    {fmt(tt)}   {100 * statistics.median(tt) / statistics.median(tf):.0f}% of the frame",
                  f"    prepare + taps + the rest  {fmt(rest)}",
                  f"  reference call structure     {fmt(tr)}   ({1 + R} calls)",
                  f"  ratio of medians             {statistics.median(tr) / statistics.median(tf):9.1f}x",
                  f"  largest |fused - reference structure| over the rows: {float((x - y.double()).abs().max()):.2e} "
                  f"(whole image {float(x[0]):.5f})"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
