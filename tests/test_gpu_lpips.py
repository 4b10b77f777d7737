"""GPU tests of the LPIPS metric (csrc/lpips.hip through gs_train.lpips and gs_train.evaluate) against
the reference-generated fixture tests/golden/lpips.npz and the fp64 restatement tests/lpips_ref.py.

Tolerances.  The bar of a row is 4 max(D, D_gpu), absolute.  D is the fixture's largest |reference fp32
- reference fp64| for the row's kind (whole image 6.8e-9, regions 1.3e-8, one-pixel regions 5.2e-9, on
values near 0.02).  D_gpu is the same distance for the torch fp32 formulation (lpips_ref in fp32 on
the GPU) on the test's own inputs: the largest over the rows of that kind in the case.  Both are
distances of the reference formulation, never of the kernels; the factor 4 is the project's standing
margin for a different summation order.  An empty region's row is exactly 0.

With GSR_LPIPS_MARGINS=<file> every comparison appends its D, D_gpu and the kernels' own distance to
that file as one JSON line (profiles/r13_lpips_margins.jsonl was made that way).
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips.npz")
DEV = "cuda:0"
NAMES = ["ones", "empty", "pixel", "blob_a", "blob_b"]


def bitwise_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(
        a.contiguous().view(torch.int64 if a.element_size() == 8 else torch.int32),
        b.contiguous().view(torch.int64 if a.element_size() == 8 else torch.int32))


def as_i16(a):
    """uint16 numpy plane -> the int16 torch plane of the same bits, on the device."""
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint16).view(np.int16)).to(DEV)


def check_rows(what, got, want, ref32, kinds, D):
    """got, want, ref32: (rows,) float64; the bar per row from D (fixture, per kind) and D_gpu =
    max |ref32 - want| over the rows of the kind.  Prints and records the figures, then asserts."""
    got, want, ref32 = (np.asarray(v, np.float64) for v in (got, want, ref32))
    fig = {}
    for kind in sorted(set(kinds) - {"empty"}):
        rows = [r for r, k in enumerate(kinds) if k == kind]
        fig[kind] = {"D": float(D[kind]), "D_gpu": float(np.abs(ref32[rows] - want[rows]).max()),
                     "kernel": float(np.abs(got[rows] - want[rows]).max()),
                     "value": float(np.abs(want[rows]).max())}
        fig[kind]["bar"] = 4 * max(fig[kind]["D"], fig[kind]["D_gpu"])
    print(what, json.dumps(fig))
    if os.environ.get("GSR_LPIPS_MARGINS"):
        with open(os.environ["GSR_LPIPS_MARGINS"], "a") as f:
            f.write(json.dumps({"test": what, **fig}) + "\n")
    for r, kind in enumerate(kinds):
        if kind == "empty":
            assert got[r] == 0.0, (what, r, got[r])
        else:
            assert abs(got[r] - want[r]) <= fig[kind]["bar"], (what, r, kind, got[r], want[r], fig[kind])


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def D(gold):
    return {k: float(gold["D_" + k]) for k in ("whole", "region", "single")}


@pytest.fixture(scope="module")
def weights():
    return lpips_ref.make_weights(0)


@pytest.fixture(scope="module")
def model(weights):
    from gs_train.lpips import LpipsModel
    return LpipsModel.from_state_dicts(*weights, device=DEV)


@pytest.fixture(scope="module")
def torch32(gold, weights):
    """Per fixture case: the (5, rows) stage terms of the torch fp32 formulation on the GPU, as fp64."""
    vgg, lin = ({k: v.to(DEV) for k, v in d.items()} for d in weights)
    out = []
    with torch.backends.cudnn.flags(enabled=False):
        for k in range(int(gold["n"])):
            t = lambda name: torch.from_numpy(gold[f"{name}_{k}"])
            masks = lpips_ref.masks_of_bits(torch.from_numpy(gold[f"bits_{k}"].astype(np.int32)), 5)
            out.append(lpips_ref.lpips_rows(t("image"), t("gt"), t("alpha"), masks, (vgg, lin), torch.float32,
                                            DEV).double().cpu().numpy())
    return out


def _lib():
    from gs_train._native import check, lib, ptr, stream
    return lib(), check, ptr, stream


def prepare(image, gt, alpha):
    L, check, ptr, stream = _lib()
    H, W = image.shape[-2:]
    out = torch.empty((2, 3, H, W), dtype=torch.float32, device=DEV)
    check(L.gsr_lpips_prepare(ptr(image), ptr(gt), ptr(alpha), H, W, ptr(out), stream(out.device)), "prepare")
    return out


def tap(feat, lin, bits, n_regions, H, W, pool=True):
    """(rows (1 + n_regions,) float64 on the device, pooled or None) of one gsr_lpips_tap call."""
    L, check, ptr, stream = _lib()
    _, C, h, w = feat.shape
    scratch = torch.empty(max(1, L.gsr_lpips_tap_scratch_bytes(h, w, n_regions)), dtype=torch.uint8, device=DEV)
    out = torch.full((1 + n_regions,), float("nan"), dtype=torch.float64, device=DEV)
    pooled = torch.full((2, C, h // 2, w // 2), float("nan"), dtype=torch.float32, device=DEV) if pool else None
    check(L.gsr_lpips_tap(ptr(feat), ptr(lin), C, h, w, ptr(bits) if n_regions else ctypes.c_void_p(0), n_regions,
                          H, W, ptr(pooled) if pool else ctypes.c_void_p(0), ptr(scratch), ptr(out),
                          stream(out.device)), "tap")
    return out, pooled


@pytest.mark.parametrize("k,with_alpha", [(0, False), (1, True), (2, True)])
def test_prepare_is_the_torch_expression_bit_for_bit(gold, k, with_alpha):
    image, gt = (torch.from_numpy(gold[f"{n}_{k}"]).to(DEV) for n in ("image", "gt"))
    alpha = torch.from_numpy(gold[f"alpha_{k}"]).to(DEV) if with_alpha else None
    got = prepare(image, gt, alpha)
    mean = torch.tensor(lpips_ref.MEAN, dtype=torch.float32, device=DEV)[None, :, None, None]
    std = torch.tensor(lpips_ref.STD, dtype=torch.float32, device=DEV)[None, :, None, None]
    a = 1.0 if alpha is None else alpha[None, None]
    want = (torch.stack([image, gt]).clamp(0.0, 1.0) * a - mean) / std
    assert bitwise_equal(got, want)
    # and it is the restatement's z-scored masked input
    x, y = lpips_ref.masked_inputs(image, gt, alpha)
    assert bitwise_equal(got[0:1], lpips_ref.z_score(x)) and bitwise_equal(got[1:2], lpips_ref.z_score(y))


# (h, w, H, W): a stage-five-like map, the fixture's stage three (both axes off the integer rule), and
# a map with several workgroups and odd sizes
TAP_SHAPES = [(5, 7, 83, 117), (26, 39, 106, 159), (33, 65, 67, 131)]
TAP_KINDS = ["whole", "region", "empty", "single", "single", "single"] + ["region"] * 11


def tap_case(C, h, w, H, W):
    """Pre-ReLU features with all-zero channel vectors in one image, the other and both, pixels and a
    row where the two images agree, and sixteen regions: all ones, empty, three single pixels (one of
    them where the images agree), and eleven random ones of mixed density."""
    g = torch.Generator().manual_seed(1000 * C + 10 * h + w)
    f = torch.randn((2, C, h, w), generator=g)
    f[0, :, 0, 0] = -f[0, :, 0, 0].abs()          # X is all zero after the ReLU
    f[:, :, 0, 1] = -f[:, :, 0, 1].abs() - 0.5    # both are
    f[1, :, 1, 0] = -f[1, :, 1, 0].abs()          # Y is
    f[1, :, h // 2, :] = f[0, :, h // 2, :]       # a row where the images agree: d = 0 exactly
    f[1, :, h - 1, w - 1] = f[0, :, h - 1, w - 1]
    lin = torch.rand(C, generator=g)
    bits = torch.randint(0, 65536, (H, W), generator=g, dtype=torch.int32)
    bits &= torch.randint(0, 65536, (H, W), generator=g, dtype=torch.int32) | 0x00FF  # bits 8..15 at 25%
    bits = (bits | 1) & ~0b11110
    src_r, src_c = lpips_ref.nearest_index(h, H), lpips_ref.nearest_index(w, W)
    for bit, (i, j) in zip((2, 3, 4), ((0, 0), (h - 1, w - 1), (h // 3, w // 2))):
        bits[src_r[i], src_c[j]] |= 1 << bit
    return f, lin, bits


@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("shape", TAP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tap_on_synthetic_features(C, shape, D):
    h, w, H, W = shape
    f, lin, bits = tap_case(C, h, w, H, W)
    fd, lind, bitsd = f.to(DEV), lin.to(DEV), as_i16(bits.numpy())
    rows, pooled = tap(fd, lind, bitsd, 16, H, W)
    assert bitwise_equal(pooled, F.max_pool2d(F.relu(fd), 2, 2)) and pooled.shape[-2:] == (h // 2, w // 2)

    masks = lpips_ref.masks_of_bits(bits, 16)
    x, y = F.relu(f[0:1]), F.relu(f[1:2])
    w4 = lin.reshape(1, C, 1, 1)
    want = [float(lpips_ref.stage_value(x.double(), y.double(), w4.double(), m)) for m in [None] + masks]
    ref32 = [float(lpips_ref.stage_value(x.to(DEV), y.to(DEV), w4.to(DEV), None if m is None else m.to(DEV)))
             for m in [None] + masks]
    assert want[3] > 0 and want[4] == 0.0 and want[2] == 0.0  # a pixel with X = 0, one with X = Y, the empty region
    got = rows.cpu().numpy()
    check_rows(f"tap C={C} {h}x{w}", got, want, ref32, TAP_KINDS, D)
    assert got[4] == 0.0  # X = Y at that pixel: exactly zero, not merely small

    # two calls give the same bits; NULL pooled_out changes nothing
    again, _ = tap(fd, lind, bitsd, 16, H, W, pool=False)
    assert bitwise_equal(rows, again)
    # a region's row does not depend on which other regions ride along
    sub = 5
    alone, _ = tap(fd, lind, bitsd, sub, H, W, pool=False)
    assert bitwise_equal(alone, rows[:1 + sub])
    shifted = as_i16(((bits >> 7) & 1).numpy())  # region 7 as the only region, bit 0
    one, _ = tap(fd, lind, shifted, 1, H, W, pool=False)
    assert bitwise_equal(one[1:], rows[8:9]) and bitwise_equal(one[:1], rows[:1])
    none, _ = tap(fd, lind, None, 0, H, W, pool=False)
    assert none.shape == (1,) and bitwise_equal(none, rows[:1])


def test_tap_of_identical_images_is_exactly_zero():
    h, w, H, W = TAP_SHAPES[2]
    f, lin, bits = tap_case(64, h, w, H, W)
    f[1] = f[0]
    rows, _ = tap(f.to(DEV), lin.to(DEV), as_i16(bits.numpy()), 16, H, W, pool=False)
    assert torch.all(rows == 0.0)


@pytest.mark.parametrize("k", range(3))
def test_frame_against_the_fixture(gold, model, torch32, D, k):
    from gs_train.evaluate import frame_metrics
    from gs_train.lpips import accumulate
    t = lambda name: torch.from_numpy(gold[f"{name}_{k}"]).to(DEV)
    bits = as_i16(gold[f"bits_{k}"])
    rows = model.frame(t("image"), t("gt"), t("alpha"), bits, 5)
    assert rows.shape == (6,) and rows.dtype == torch.float64 and rows.is_cuda
    kinds = [str(v) for v in gold["kinds"]]
    check_rows(f"frame {tuple(gold[f'alpha_{k}'].shape)}", rows.cpu().numpy(), gold[f"ref64_{k}"],
               torch32[k].sum(0), kinds, D)
    assert bitwise_equal(rows, model.frame(t("image"), t("gt"), t("alpha"), bits, 5))
    assert bitwise_equal(rows[:1], model.frame(t("image"), t("gt"), t("alpha")))  # no regions
    # the empty region is reported as not evaluated by the frame table, and accumulate skips it
    table = frame_metrics(t("image"), t("gt"), t("alpha"), None, None, bits, 5)
    assert table[2, 5] == 0 and torch.all(table[[0, 1, 3, 4, 5], 5] == 1)
    tot = torch.zeros((6, 2), dtype=torch.float64, device=DEV)
    accumulate(rows, table, tot)
    accumulate(rows, table, tot)
    want = torch.stack([2 * table[:, 4] * rows, 2 * table[:, 4]], 1)
    want[2] = 0
    assert torch.equal(tot, want) and torch.all(tot[2] == 0) and tot[0, 1] == 2 * bits.numel()


def test_frame_size_and_device_errors(model):
    z = torch.zeros((3, 15, 40), device=DEV)
    with pytest.raises(ValueError, match="16"):
        model.frame(z, z)


def test_evaluator_with_a_model_over_three_frames(gold, model, weights, torch32, D):
    """The pixel-weighted LPIPS per row against the fp64 restatement's, and every other column
    bit-identical to an Evaluator without a model."""
    from gs_train.evaluate import Evaluator
    ev, plain = Evaluator(NAMES, lpips=model), Evaluator(NAMES)
    num64, num32, den = np.zeros(6), np.zeros(6), np.zeros(6)
    for k in range(3):
        t = lambda name: torch.from_numpy(gold[f"{name}_{k}"])
        bits = as_i16(gold[f"bits_{k}"])
        args = [t(n).to(DEV) for n in ("image", "gt", "alpha")]
        frame = ev.add(*args, region_bits=bits)
        assert bitwise_equal(frame, plain.add(*args, region_bits=bits))
        masks = lpips_ref.masks_of_bits(torch.from_numpy(gold[f"bits_{k}"].astype(np.int32)), 5)
        l64 = lpips_ref.lpips_rows(t("image"), t("gt"), t("alpha"), masks, weights, torch.float64).sum(0).numpy()
        wt = frame[:, 4].cpu().numpy() * (frame[:, 5].cpu().numpy() != 0)
        num64 += wt * l64
        num32 += wt * torch32[k].sum(0)
        den += wt
    assert bitwise_equal(ev.totals, plain.totals)
    assert np.array_equal(ev.lpips_totals[:, 1].cpu().numpy(), den) and den[2] == 0 and den[0] > 0
    res, base = ev.result(), plain.result()
    kinds = [str(v) for v in gold["kinds"]]
    live = [r for r in range(6) if den[r] > 0]
    got = np.array([res[n]["lpips"] if res[n]["lpips"] is not None else 0.0 for n in ["whole_image"] + NAMES])
    assert res["empty"]["lpips"] is None and res["empty"]["image_count"] == 0 and live == [0, 1, 3, 4, 5]
    safe = np.maximum(den, 1)
    check_rows("evaluator, three frames", got, num64 / safe, num32 / safe, kinds, D)
    for n in ["whole_image"] + NAMES:
        assert {k: v for k, v in res[n].items() if k != "lpips"} == base[n]
    lines, plain_lines, rows = ev.format(), plain.format(), ["whole_image"] + NAMES
    assert len(lines) == len(plain_lines) == len(rows) and lines[0].startswith("Whole Image: PSNR: ")
    assert [ln.replace(f" LPIPS: {res[n]['lpips']:.5f}", "") if res[n]["lpips"] is not None else ln
            for ln, n in zip(lines, rows)] == plain_lines
    assert all(ln.index(" SSIM: ") < ln.index(" LPIPS: ") < ln.index(" iMAE: ")
               for ln, n in zip(lines, rows) if n != "empty")


@pytest.mark.timeout(120)
def test_street_sized_frame_with_nine_regions(model):
    """One 1536x1536 frame with the standard nine regions: runs, finite, rows in range."""
    g = torch.Generator(device=DEV).manual_seed(3)
    H = W = 1536
    image = torch.rand((3, H, W), generator=g, device=DEV)
    gt = (image + 0.05 * torch.randn((3, H, W), generator=g, device=DEV)).clamp(0, 1)
    bits = torch.randint(0, 512, (H, W), generator=g, device=DEV, dtype=torch.int32).to(torch.int16)
    rows = model.frame(image, gt, None, bits, 9).cpu()
    assert rows.shape == (10,) and torch.isfinite(rows).all() and (rows > 0).all() and (rows < 5).all()
    assert abs(float(rows[1] / rows[0]) - 1) < 0.05  # a random half of the pixels: close to the whole image
