"""GPU tests of the fused evaluation metrics (csrc/eval.hip through gs_train.evaluate) against the
reference-generated fixture tests/golden/eval.npz and the fp64 restatement tests/eval_ref.py.

Tolerances: max(floor, 4 D) per quantity and kind of region (eval_ref.tolerances), D the largest
|reference fp32 - reference fp64| the fixture records (the factor 4: the kernel's summation order
differs from conv2d's).  D for one-pixel regions: 2.3e-6 dB (PSNR), 2.7e-5 (SSIM), 0 (iMAE, iRMSE);
for every other row 2.1e-6 dB, 2.4e-7, 1.9e-7 and 5.9e-8 relative.  Floors: 1e-5 dB (PSNR), 2e-6
(SSIM, the bar of test_gpu_train.py against loss.npz), 1e-6 relative (iMAE, iRMSE): they govern
every row but the one-pixel regions' SSIM (1.1e-4).
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_ref  # noqa: E402
import helpers  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval.npz")
DEV = "cuda:0"


def bitwise_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def as_i16(a):
    """uint16 numpy plane -> the int16 torch plane of the same bits, on the device."""
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint16).view(np.int16)).to(DEV)


def report(what, got, want):
    """The figures behind an assertion, printed before it (pytest -s / the job log)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got[:, :4] - want[:, :4])
    err[:, 2:] /= np.maximum(np.abs(want[:, 2:4]), 1e-300)
    print(f"{what}: max error per row (psnr dB, ssim, imae rel, irmse rel)")
    for r in range(len(err)):
        print("   row", r, " ".join(f"{e:.3e}" for e in err[r]))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def frame70():
    """One 70x130 frame with sixteen overlapping random regions of mixed density."""
    g = torch.Generator().manual_seed(5)
    H, W = 70, 130
    img = torch.rand((3, H, W), generator=g) * 1.2 - 0.1
    gt = img + 0.1 * torch.randn((3, H, W), generator=g)
    alpha = (torch.rand((H, W), generator=g) >= 0.1).float()
    gt_invd = torch.rand((H, W), generator=g) * 0.4
    invd = gt_invd + 0.02 * torch.randn((H, W), generator=g)
    bits = torch.randint(0, 65536, (H, W), generator=g, dtype=torch.int32)
    bits &= torch.randint(0, 65536, (H, W), generator=g, dtype=torch.int32) | 0x00FF  # bits 8..15 at 25%
    bits[20:40, 60:70] &= 0xFFFE  # region 0 has a hole across a tile border
    d = lambda t: t.to(DEV)
    return dict(img=d(img), gt=d(gt), alpha=d(alpha), invd=d(invd), gt_invd=d(gt_invd), bits=as_i16(bits.numpy()),
                bits_cpu=bits, cpu=(img, gt, alpha, invd, gt_invd))


@pytest.mark.parametrize("k", range(4))
def test_fixture_parity(gold, k):
    from gs_train.evaluate import frame_metrics
    t = lambda name: torch.from_numpy(gold[f"{name}_{k}"]).to(DEV)
    table = frame_metrics(t("image"), t("gt"), t("alpha"), t("invdepth"), t("gt_invdepth"),
                          as_i16(gold[f"bits_{k}"]), 5).cpu()
    ref64 = gold[f"ref64_{k}"]
    kinds = ["single" if s else "other" for s in gold[f"single_{k}"]]
    report(f"case {k} {tuple(gold[f'alpha_{k}'].shape)} against the reference in fp64", table.numpy(), ref64)
    eval_ref.check_rows(table, ref64, kinds, eval_ref.tolerances(gold), f"case {k}")
    assert np.array_equal(table[:, 4].numpy(), ref64[:, 4])  # weights
    assert torch.all(table[:, 5] == 1)
    masks = eval_ref.masks_of_bits(torch.from_numpy(gold[f"bits_{k}"].astype(np.int32)), 5)
    npix = gold[f"alpha_{k}"].size
    assert table[:, 6].tolist() == [npix] + [int(m.sum()) for m in masks]
    assert torch.equal(table[:, 7], table[:, 6])


def _ulp_neighbours(x, n=24):
    x = np.float32(x)
    out = [x]
    lo = hi = x
    for _ in range(n):
        lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(1))
        out += [lo, hi]
    return out


def test_depth_range_bits_are_torch_exact():
    from gs_train.evaluate import DEPTH_RANGES, depth_range_bits
    g = torch.Generator().manual_seed(3)
    H, W = 37, 53
    inv = torch.rand((H, W), generator=g) * 0.4
    edge = [v for t in (5.0, 20.0) for v in _ulp_neighbours(1.0 / t - 1e-6)] + [0.0, 1e-9, 1.0, 1e6]
    inv.view(-1)[:len(edge)] = torch.tensor(np.array(edge, np.float32))
    depth = (1.0 / (inv + 1e-6)).view(-1)[:len(edge)]
    for t in (5.0, 20.0):  # the fp32 depth lands on the boundary and one ulp either side
        for v in (t, np.nextafter(np.float32(t), np.float32(0)), np.nextafter(np.float32(t), np.float32(100))):
            assert bool((depth == float(v)).any()), f"no inverse depth gives the depth {v!r}"
    want = torch.zeros((H, W), dtype=torch.int32)
    for r, (lo, hi) in enumerate(DEPTH_RANGES):
        want |= eval_ref.depth_range_mask(inv, lo, hi).to(torch.int32) << r
    got = depth_range_bits(inv.to(DEV))
    assert got.dtype == torch.int16 and torch.equal(got.cpu().to(torch.int32), want)
    assert int((want == 0).sum()) == 0  # the three ranges cover every depth
    # shift > 0 into a non-empty plane: the old bits stay
    old = torch.randint(0, 8, (H, W), generator=g, dtype=torch.int32)
    plane = as_i16(old.numpy())
    out = depth_range_bits(inv.to(DEV), ((0.0, 5.0), (20.0, math.inf)), bits=plane, shift=13)
    assert out is plane
    want2 = old | (eval_ref.depth_range_mask(inv, 0.0, 5.0).to(torch.int32) << 13) \
        | (eval_ref.depth_range_mask(inv, 20.0, math.inf).to(torch.int32) << 14)
    assert torch.equal(plane.cpu().to(torch.int32) & 0xFFFF, want2)


def test_category_bits_are_torch_exact():
    from gs_train.evaluate import CATEGORY_COLORS, category_bits
    g = torch.Generator().manual_seed(4)
    H, W = 37, 53
    colors = list(CATEGORY_COLORS.values())
    near = [(135, 206, 234), (135, 207, 235), (0, 0, 0), (255, 215, 1)]  # one channel off, and unlabelled
    table = torch.tensor(colors + near, dtype=torch.uint8)
    seg = table[torch.randint(0, len(table), (H, W), generator=g)].permute(2, 0, 1).contiguous()
    want = torch.zeros((H, W), dtype=torch.int32)
    for r, c in enumerate(colors):
        want |= eval_ref.color_mask(seg, c).to(torch.int32) << r
    got = category_bits(seg.to(DEV))
    assert torch.equal(got.cpu().to(torch.int32), want) and int((want == 0).sum()) > 0
    rgba = torch.cat([seg, torch.full((1, H, W), 255, dtype=torch.uint8)])
    plane = torch.full((H, W), 5, dtype=torch.int16, device=DEV)
    category_bits(rgba.to(DEV), colors, bits=plane, shift=3)
    assert torch.equal(plane.cpu().to(torch.int32), (want << 3) | 5)


def test_regions_do_not_leak_into_each_other(frame70):
    """Sixteen overlapping regions in one call: each row is bitwise the row of a call that carries
    only that region, and row 0 is the row of a call without regions.  Two calls give the same bits."""
    from gs_train.evaluate import frame_metrics
    f = frame70
    full = frame_metrics(f["img"], f["gt"], f["alpha"], f["invd"], f["gt_invd"], f["bits"], 16)
    again = frame_metrics(f["img"], f["gt"], f["alpha"], f["invd"], f["gt_invd"], f["bits"], 16)
    assert bitwise_equal(full, again)
    none = frame_metrics(f["img"], f["gt"], f["alpha"], f["invd"], f["gt_invd"])
    assert none.shape == (1, 8) and bitwise_equal(full[:1], none)
    assert torch.all(full[:, 5] == 1) and torch.isfinite(full).all()
    for r in range(16):
        one = as_i16(((f["bits_cpu"] >> r) & 1).numpy())
        alone = frame_metrics(f["img"], f["gt"], f["alpha"], f["invd"], f["gt_invd"], one, 1)
        assert bitwise_equal(full[1 + r:2 + r], alone[1:]), f"region {r}"
    # and the rows are the right ones
    img, gt, alpha, invd, gt_invd = f["cpu"]
    want = eval_ref.frame_table(img, gt, alpha, invd, gt_invd, eval_ref.masks_of_bits(f["bits_cpu"], 16))
    report("sixteen regions at 70x130 against eval_ref", full.cpu().numpy(), want.numpy())
    tol = {"other": (1e-5, 2e-6, 1e-6, 1e-6)}
    eval_ref.check_rows(full.cpu(), want, ["other"] * 17, tol, "sixteen regions")
    assert torch.equal(full[:, 4:].cpu(), want[:, 4:])


def test_empty_region_and_zero_alpha(frame70):
    from gs_train.evaluate import Evaluator
    f = frame70
    bits = as_i16((f["bits_cpu"] & 0b101).numpy())  # region 1 is empty
    ev = Evaluator(["a", "empty", "c"])
    frame = ev.add(f["img"], f["gt"], f["alpha"], f["invd"], f["gt_invd"], bits)
    assert torch.all(frame[2] == 0) and frame[1, 5] == 1 and frame[3, 5] == 1
    assert torch.all(ev.totals[2] == 0) and ev.totals[1, 5] == 1
    res = ev.result()
    assert res["empty"]["image_count"] == 0 and res["empty"]["psnr"] is None and res["a"]["image_count"] == 1
    assert "  Region 'empty' : Not found or no valid overlap in any evaluated image." in ev.format()
    # all-zero alpha: x = y = 0 everywhere
    ev0 = Evaluator(["a", "empty", "c"])
    frame = ev0.add(f["img"], f["gt"], torch.zeros_like(f["alpha"]), f["invd"], f["gt_invd"], bits)
    assert frame[0, 2] == 0 and frame[0, 3] == 0 and frame[0, 0] == math.inf and frame[0, 1] == 1
    assert frame[1, 5] == 1 and frame[1, 4] == 0  # evaluated, weight 0: left out of the sums
    assert not torch.isnan(ev0.totals).any()
    assert torch.all(ev0.totals[1:] == 0) and ev0.totals[0, 5] == 1 and ev0.totals[0, 4] == 70 * 130


def test_null_forms_match_explicit_inputs(frame70):
    from gs_train.evaluate import frame_metrics
    f = frame70
    ones = torch.ones_like(f["alpha"])
    a = frame_metrics(f["img"], f["gt"], None, f["invd"], f["gt_invd"], f["bits"], 4)
    b = frame_metrics(f["img"], f["gt"], ones.unsqueeze(0), f["invd"], f["gt_invd"], f["bits"], 4)
    assert bitwise_equal(a, b)
    a = frame_metrics(f["img"], f["gt"], f["alpha"], None, None, f["bits"], 4)
    b = frame_metrics(f["img"], f["gt"], f["alpha"], ones, ones, f["bits"], 4)
    assert bitwise_equal(a, b) and torch.all(a[:, 2:4] == 0)


def test_accumulate_is_the_fp64_sum(frame70):
    from gs_train.evaluate import Evaluator
    f = frame70
    ev = Evaluator([f"r{i}" for i in range(6)])
    frames = []
    for s in range(3):
        img = torch.roll(f["img"], s * 7, dims=2)
        bits = as_i16(((f["bits_cpu"] >> s) & (0x3F if s else 0x3D)).numpy())  # frame 0: region 1 empty
        frames.append(ev.add(img, f["gt"], f["alpha"], f["invd"], f["gt_invd"], bits).cpu())
    want = torch.zeros((7, 6), dtype=torch.float64)
    for fr in frames:
        want = eval_ref.accumulate(want, fr)
    assert bitwise_equal(ev.totals.cpu(), want)
    assert want[:, 5].tolist() == [3, 3, 2, 3, 3, 3, 3]


def test_evaluator_end_to_end_on_rendered_views():
    """Three views of a synthetic scene against the renders of a perturbed copy, through add_view
    (one with the right-half crop), against eval_ref on the same maps."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from gs_train import synthetic
    from gs_train.evaluate import DEPTH_RANGES, Evaluator
    W, H, P = 96, 64, 2000
    scene = synthetic.synthetic_scene(P, W, H, seed=1, log_scale_mean=-3.0)
    rng = np.random.default_rng(2)
    other = dict(scene)
    other["means3D"] = (scene["means3D"] + rng.normal(0, 0.02, (P, 3))).astype(np.float32)
    other["shs"] = (scene["shs"] + rng.normal(0, 0.05, scene["shs"].shape)).astype(np.float32)
    ev = Evaluator()
    want = torch.zeros((4, 6), dtype=torch.float64)
    tg = torch.Generator().manual_seed(9)
    for v, cam in enumerate(synthetic.orbit_cameras(3, W, H)):
        maps = []
        for sc in (scene, other):
            sc = dict(sc, view=cam[0], proj=cam[1], campos=cam[2], tanfovx=cam[3], tanfovy=cam[4])
            with torch.no_grad():
                color, _, invd = GaussianRasterizer(helpers.settings(sc, DEV, 3))(
                    **helpers.torch_inputs(sc, DEV, requires_grad=False))
            maps += [color, invd]
        alpha = (torch.rand((1, H, W), generator=tg) >= 0.1).float()
        view = dict(original_image=maps[2], alpha_mask=alpha, invdepthmap=maps[3])
        half = v == 1
        frame = ev.add_view({"render": maps[0], "depth": maps[1]}, view, half=half).cpu()
        crop = (lambda t: t[..., W // 2:]) if half else (lambda t: t)
        img, invd, gt, gt_invd = [crop(m.cpu()) for m in maps]
        masks = [eval_ref.depth_range_mask(gt_invd, lo, hi) for lo, hi in DEPTH_RANGES]
        ref = eval_ref.frame_table(img, gt, crop(alpha), invd, gt_invd, masks)
        report(f"view {v} (half={half}) against eval_ref", frame.numpy(), ref.numpy())
        print("   mask pixels", ref[:, 6].tolist(), "weights", ref[:, 4].tolist())
        assert torch.equal(frame[:, 4:7], ref[:, 4:7])
        assert frame[0, 4] == H * (W // 2 if half else W)
        want = eval_ref.accumulate(want, ref)
    assert want[0, 5] == 3 and (want[1:, 5] > 0).sum() >= 2  # the scene spans several depth ranges
    res = ev.result()
    names = ["whole_image", "depth_near", "depth_medium", "depth_far"]
    got_rows, want_rows = [], []
    for r, name in enumerate(names):
        assert res[name]["image_count"] == int(want[r, 5]) and res[name]["pixel_count"] == int(want[r, 4])
        if res[name]["image_count"]:
            got_rows.append([res[name][c] for c in ("psnr", "ssim", "imae", "irmse")])
            want_rows.append((want[r, :4] / want[r, 4]).tolist())
    report("the test set's result()", got_rows, want_rows)
    eval_ref.check_rows(got_rows, want_rows, ["other"] * len(got_rows), {"other": (1e-5, 2e-6, 1e-6, 1e-6)}, "result")
    assert ev.format()[0].startswith("Whole Image: PSNR: ")
