"""CPU tests of the evaluation metrics (gs_train.evaluate, include/gsr_eval.h): the ctypes table
against the header and the library, tests/eval_ref.py against the reference-generated fixture
(tests/golden/eval.npz), the argument errors, and the report from a hand-made totals table.

Tolerances: max(floor, 4 D) per quantity and kind of region (eval_ref.tolerances), D the largest
|reference fp32 - reference fp64| the fixture records: for one-pixel regions 2.3e-6 dB (PSNR) and
2.7e-5 (SSIM), for every other row 2.1e-6 dB, 2.4e-7, 1.9e-7 and 5.9e-8 (PSNR, SSIM, iMAE and iRMSE
relative).  Floors: 1e-5 dB, 2e-6, 1e-6 and 1e-6 relative.
"""
from __future__ import annotations

import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gsr_eval.h")
GOLD = os.path.join(REPO, "tests", "golden", "eval.npz")
ENTRY_POINTS = {"gsr_eval_depth_range_bits", "gsr_eval_color_bits", "gsr_eval_frame_scratch_bytes", "gsr_eval_frame",
                "gsr_eval_accumulate"}


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(gsr_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out


def test_lib_declares_the_header_entry_points():
    from diff_gaussian_rasterization import _lib
    decl = _declarations()
    assert set(decl) == ENTRY_POINTS
    table = getattr(_lib, "EVAL_SIGNATURES", {})
    assert set(table) == set(decl), "ctypes table out of sync with include/gsr_eval.h"
    for name, n in decl.items():
        assert len(table[name][1]) == n, f"{name}: {len(table[name][1])} ctypes arguments, the header has {n}"
    assert not set(table) & (set(_lib.SIGNATURES) | set(_lib.GT_SIGNATURES))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), f"libgsr_hip.so does not export {name}"
    L = _lib.load()
    assert L.gsr_eval_frame_scratch_bytes.restype is ctypes.c_size_t
    assert L.gsr_abi_version() == 7


def test_native_calls_validate_without_gpu():
    """Argument checks return before any device work."""
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    assert L.gsr_eval_frame_scratch_bytes(0, 5, 0) == 0 and L.gsr_eval_frame_scratch_bytes(5, 5, 17) == 0
    # ten fp32 sums per row and 64x16 tile
    assert L.gsr_eval_frame_scratch_bytes(70, 130, 5) == 4 * 10 * 6 * 3 * 5
    assert L.gsr_eval_frame(None, None, None, None, None, None, 0, 4, 4, None, None, None) != 0
    assert b"gsr_eval_frame" in L.gsr_last_error()
    one = ctypes.c_void_p(16)  # never dereferenced: the call fails on its arguments
    assert L.gsr_eval_frame(one, one, None, None, None, None, 17, 4, 4, one, one, None) != 0
    assert L.gsr_eval_frame(one, one, None, None, None, None, 2, 4, 4, one, one, None) != 0  # regions, no bits
    assert L.gsr_eval_frame(one, one, None, one, None, None, 0, 4, 4, one, one, None) != 0  # half a depth pair
    assert L.gsr_eval_accumulate(None, 1, None, None) != 0
    assert L.gsr_eval_accumulate(one, 18, one, None) != 0
    lo = (ctypes.c_float * 1)(0.0)
    assert L.gsr_eval_depth_range_bits(one, 4, 1, lo, lo, 16, one, None) != 0  # bit 16
    col = (ctypes.c_uint8 * 3)(1, 2, 3)
    assert L.gsr_eval_color_bits(one, 4, 1, col, -1, one, None) != 0


def _cases():
    g = np.load(GOLD)
    return g, range(int(g["n"]))


def test_fixture_shapes_and_margins():
    g, ks = _cases()
    assert [tuple(g[f"alpha_{k}"].shape) for k in ks] == [(7, 9), (16, 16), (37, 53), (70, 130)]
    assert float(g["min_window_weight"]) >= 1.05e-6 and float(g["min_denominator"]) >= 1e-8
    for k in ks:
        a = g[f"alpha_{k}"]
        assert 0.02 < float((a == 0).mean()) < 0.25 and a[0, 0] == 1
        bits = g[f"bits_{k}"]
        assert bits.dtype == np.uint16 and int(bits[0, 0]) & 16 and int((bits & 16 != 0).sum()) == 1
        assert list(g[f"single_{k}"]) == [False] * 5 + [True]
        assert float(g[f"gt_invdepth_{k}"].min()) >= 0 and float(g[f"gt_invdepth_{k}"].max()) < 0.4
        assert (g[f"image_{k}"] < 0).any() and (g[f"image_{k}"] > 1).any()  # unclamped inputs
    tol = eval_ref.tolerances(g)
    # the floors govern ordinary rows (the reference's own fp32 error there is well below them)
    assert tol["other"] == (1e-5, 2e-6, 1e-6, 1e-6)
    assert tol["single"][1] == pytest.approx(4 * float(g["D_single"][1])) and 2e-6 < tol["single"][1] < 2e-4


@pytest.mark.parametrize("k", range(4))
def test_eval_ref_reproduces_the_fixture(k):
    """The fp64 restatement against what the reference's functions returned, in fp32 and in fp64, and
    its depth-range masks against the reference's bit for bit."""
    g, _ = _cases()
    t = lambda name: torch.from_numpy(g[f"{name}_{k}"])
    bits = torch.from_numpy(g[f"bits_{k}"].astype(np.int32))
    masks = eval_ref.masks_of_bits(bits, 5)
    for r, (lo, hi) in enumerate([(0.0, 5.0), (5.0, 20.0), (20.0, math.inf)]):
        assert torch.equal(eval_ref.depth_range_mask(t("gt_invdepth"), lo, hi), masks[r])
    table = eval_ref.frame_table(t("image"), t("gt"), t("alpha"), t("invdepth"), t("gt_invdepth"), masks)
    kinds = ["single" if s else "other" for s in g[f"single_{k}"]]
    tol = eval_ref.tolerances(g)
    ref64, ref32 = g[f"ref64_{k}"], g[f"ref32_{k}"]
    eval_ref.check_rows(table, ref32, kinds, tol, "fp32 reference")
    exact = {kind: (1e-9, 1e-10, 1e-10, 1e-10) for kind in tol}  # fp64 against fp64: summation order only
    eval_ref.check_rows(table, ref64, kinds, exact, "fp64 reference")
    assert np.array_equal(table[:, 4].numpy(), ref64[:, 4])
    assert torch.all(table[:, 5] == 1)
    assert np.array_equal(table[:, 6].numpy(), [bits.numel()] + [int(m.sum()) for m in masks])
    assert torch.equal(table[:, 7], table[:, 6])  # a 0/1 mask's own pixels always have a valid window


def test_eval_ref_empty_region_and_accumulate():
    torch.manual_seed(0)
    img, gt = torch.rand(3, 8, 8), torch.rand(3, 8, 8)
    table = eval_ref.frame_table(img, gt, None, None, None, [torch.zeros(8, 8, dtype=torch.bool)])
    assert torch.all(table[1] == 0) and table[0, 2] == 0 and table[0, 3] == 0
    tot = eval_ref.accumulate(torch.zeros(2, 6, dtype=torch.float64), table)
    assert torch.all(tot[1] == 0) and tot[0, 4] == 64 and tot[0, 5] == 1 and tot[0, 0] == 64 * table[0, 0]


def test_frame_metrics_argument_errors_without_gpu():
    """Every argument error is a ValueError raised before any GPU call (the tensors are on the CPU)."""
    from gs_train.evaluate import category_bits, depth_range_bits, frame_metrics
    img = torch.zeros(3, 6, 8)
    plane = torch.zeros(6, 8)
    bits = torch.zeros(6, 8, dtype=torch.int16)
    with pytest.raises(ValueError):
        frame_metrics(img, torch.zeros(3, 6, 9))
    with pytest.raises(ValueError):
        frame_metrics(torch.zeros(1, 6, 8), torch.zeros(1, 6, 8))
    with pytest.raises(ValueError):
        frame_metrics(img, img, torch.zeros(8, 6))
    with pytest.raises(ValueError):
        frame_metrics(img, img, plane, invdepth=plane)
    with pytest.raises(ValueError):
        frame_metrics(img, img, plane, plane, torch.zeros(6, 7))
    with pytest.raises(ValueError):
        frame_metrics(img, img, plane, region_bits=bits.to(torch.int32), n_regions=2)
    with pytest.raises(ValueError):
        frame_metrics(img, img, plane, region_bits=torch.zeros(6, 9, dtype=torch.int16), n_regions=2)
    with pytest.raises(ValueError):
        frame_metrics(img, img, plane, region_bits=bits, n_regions=17)
    with pytest.raises(ValueError):
        frame_metrics(img, img, plane, region_bits=None, n_regions=1)
    with pytest.raises(ValueError):
        depth_range_bits(plane, bits=bits, shift=14)
    with pytest.raises(ValueError):
        depth_range_bits(plane, bits=bits.float())
    with pytest.raises(ValueError):
        category_bits(torch.zeros(3, 6, 8), bits=bits)  # not uint8
    with pytest.raises(ValueError):
        category_bits(torch.zeros(3, 6, 8, dtype=torch.uint8), bits=bits, shift=11)
    # valid arguments on the CPU: refused as not on a GPU, not as a ValueError
    with pytest.raises(RuntimeError):
        frame_metrics(img, img, plane, plane, plane, bits, 3)


def test_category_colours_are_the_reference_table():
    from gs_train.evaluate import CATEGORY_COLORS, DEPTH_RANGES
    assert list(CATEGORY_COLORS) == ["sky", "ground", "buildings", "vehicles", "vegetation", "lamposts"]
    assert CATEGORY_COLORS["sky"] == (135, 206, 235) and CATEGORY_COLORS["lamposts"] == (255, 215, 0)
    assert DEPTH_RANGES == ((0.0, 5.0), (5.0, 20.0), (20.0, math.inf))


def test_evaluator_result_and_format_from_totals():
    from gs_train.evaluate import Evaluator
    ev = Evaluator(categories=True)
    assert ev.region_names[:3] == ["depth_near", "depth_medium", "depth_far"] and ev.n_regions == 9
    tot = torch.zeros(10, 6, dtype=torch.float64)
    tot[0] = torch.tensor([2.0 * 25.0 * 100, 2.0 * 0.9 * 100, 2.0 * 0.01 * 100, 2.0 * 0.02 * 100, 200.0, 2.0])
    tot[1] = torch.tensor([30.0 * 40, 0.95 * 40, 0.5 * 40, 0.25 * 40, 40.0, 1.0])
    tot[3] = torch.tensor([math.inf, 1.0 * 7, 0.0, 0.0, 7.0, 2.0])
    tot[4] = torch.tensor([21.5 * 10, 0.5 * 10, 0.125 * 10, 0.25 * 10, 10.0, 1.0])
    res = ev.result(tot)
    assert list(res) == ["whole_image"] + ev.region_names
    assert res["whole_image"] == {"psnr": 25.0, "ssim": 0.9, "imae": 0.01, "irmse": 0.02, "pixel_count": 200,
                                  "image_count": 2}
    assert res["depth_near"]["psnr"] == 30.0 and res["depth_near"]["pixel_count"] == 40
    assert res["depth_medium"] == {"psnr": None, "ssim": None, "imae": None, "irmse": None, "pixel_count": 0,
                                   "image_count": 0}
    assert res["depth_far"]["psnr"] == math.inf and res["depth_far"]["image_count"] == 2
    assert ev.format(tot) == [
        "Whole Image: PSNR: 25.00000 SSIM: 0.90000 iMAE: 0.01000 iRMSE: 0.02000 "
        "(pixel-weighted and evaluated on 2 images)",
        "",
        "Depth-Stratified Results:",
        "  Near (0.0-5.0m): PSNR: 30.00000 SSIM: 0.95000 iMAE: 0.50000 iRMSE: 0.25000 "
        "(pixel-weighted and evaluated on 1 instances)",
        "  Medium (5.0-20.0m): No valid pixels found in this depth range.",
        "  Far (20.0m+): PSNR: inf SSIM: 1.00000 iMAE: 0.00000 iRMSE: 0.00000 "
        "(pixel-weighted and evaluated on 2 instances)",
        "",
        "Category-Specific Results:",
        "  Category 'sky' : PSNR: 21.50000 SSIM: 0.50000 iMAE: 0.12500 iRMSE: 0.25000 "
        "(pixel-weighted and evaluated on 1 images)",
    ] + [f"  Category '{n}' : Not found or no valid overlap in any evaluated image."
         for n in ["ground", "buildings", "vehicles", "vegetation", "lamposts"]]
    # nothing added yet: every row empty, no device needed
    empty = Evaluator(["a", "b"])
    assert empty.result()["a"]["image_count"] == 0
    assert empty.format() == ["  Region 'a' : Not found or no valid overlap in any evaluated image.",
                              "  Region 'b' : Not found or no valid overlap in any evaluated image."]
    with pytest.raises(ValueError):
        Evaluator([str(i) for i in range(17)])
