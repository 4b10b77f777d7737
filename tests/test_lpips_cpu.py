"""CPU tests of the LPIPS metric (gs_train.lpips, include/gsr_lpips.h): the generated weights and
tests/lpips_ref.py against the reference-generated fixture (tests/golden/lpips.npz), the ctypes table
against the header and the library, the state-dict key mapping, and the Evaluator's report with and
without a model.

Tolerances: the fp64 restatement against the reference in fp64 differs only in summation order (1e-12
absolute on values of 0.02); the fp32 restatement is held to 4 D, D the largest |reference fp32 -
reference fp64| the fixture records per kind of row: 6.8e-9 (whole image), 1.3e-8 (regions) and 5.2e-9
(the one-pixel region).
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
import lpips_ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gsr_lpips.h")
GOLD = os.path.join(REPO, "tests", "golden", "lpips.npz")
ENTRY_POINTS = {"gsr_lpips_prepare", "gsr_lpips_tap_scratch_bytes", "gsr_lpips_tap", "gsr_lpips_accumulate"}
SIZES = [(16, 16), (37, 53), (106, 159)]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def weights():
    return lpips_ref.make_weights(0)


def test_generated_weights_match_the_fixture_checksums(gold, weights):
    names, sums = lpips_ref.weight_checksums(*weights)
    assert names == list(gold["weight_names"]) and len(names) == 26 + 5
    assert np.array_equal(sums, gold["weight_sums"]), "make_weights drifted from the stream the fixture was made with"
    vgg, lin = weights
    assert all(float(t.min()) >= 0 for t in lin.values())
    assert tuple(vgg["features.28.weight"].shape) == (512, 512, 3, 3)


def test_fixture_shapes_and_regions(gold):
    assert int(gold["n"]) == 3 and list(gold["kinds"]) == ["whole", "region", "empty", "single", "region", "region"]
    for k, hw in enumerate(SIZES):
        bits, alpha = gold[f"bits_{k}"], gold[f"alpha_{k}"]
        assert bits.shape == hw and bits.dtype == np.uint16 and alpha.shape == hw
        assert (bits & 1).all() and not (bits & 2).any() and int((bits & 4 != 0).sum()) == 1 and bits[5, 7] & 4
        assert ((bits & 8 != 0) & (bits & 16 != 0)).any()  # the blobs overlap
        assert 0 < (alpha == 0).sum() < alpha.size / 4
        assert (gold[f"image_{k}"] < 0).any() and (gold[f"image_{k}"] > 1).any()  # unclamped inputs
        assert gold[f"stages64_{k}"].shape == (5, 6)
        assert np.allclose(gold[f"stages64_{k}"].sum(0), gold[f"ref64_{k}"], rtol=0, atol=1e-15)
        assert gold[f"ref64_{k}"][2] == 0 and (gold[f"stages64_{k}"][1:, 3] == 0).all()  # the 1e-8 clamp ran
    for kind in ("whole", "region", "single"):
        assert 1e-10 < float(gold["D_" + kind]) < 1e-6


@pytest.mark.parametrize("k", range(3))
def test_restatement_reproduces_the_fixture(gold, weights, k):
    t = lambda name: torch.from_numpy(gold[f"{name}_{k}"])
    masks = lpips_ref.masks_of_bits(torch.from_numpy(gold[f"bits_{k}"].astype(np.int32)), 5)
    st64 = lpips_ref.lpips_rows(t("image"), t("gt"), t("alpha"), masks, weights, torch.float64).numpy()
    assert np.abs(st64 - gold[f"stages64_{k}"]).max() <= 1e-12
    assert np.abs(st64.sum(0) - gold[f"ref64_{k}"]).max() <= 1e-12
    st32 = lpips_ref.lpips_rows(t("image"), t("gt"), t("alpha"), masks, weights, torch.float32).double().numpy()
    for r, kind in enumerate(gold["kinds"]):
        tol = 0.0 if kind == "empty" else 4 * float(gold["D_" + str(kind)])
        assert abs(st32[:, r].sum() - gold[f"ref64_{k}"][r]) <= tol, (r, kind, st32[:, r].sum(), gold[f"ref64_{k}"][r])
    # the one-call-per-row form is the same computation
    x, y = lpips_ref.masked_inputs(t("image").double(), t("gt").double(), t("alpha").double())
    assert float(lpips_ref.lpips_call(x, y, weights, masks[3])) == pytest.approx(st64[:, 4].sum(), abs=1e-15)


def test_nearest_rule_is_not_the_integer_rule():
    """The 106x159 case at stage three (26x39): torch's fp32 rule and i * H // h differ on both axes,
    so the fixture exercises the rule; and the restatement's rule is torch's."""
    assert (lpips_ref.nearest_index(26, 106) != lpips_ref.integer_index(26, 106)).sum() >= 1
    assert (lpips_ref.nearest_index(39, 159) != lpips_ref.integer_index(39, 159)).sum() >= 2
    for n_out, n_in in [(26, 106), (39, 159), (16, 16), (18, 37), (13, 53), (1, 16), (96, 1536), (7, 100)]:
        src = torch.arange(n_in, dtype=torch.float32)[None, None, None]
        got = torch.nn.functional.interpolate(src, size=(1, n_out), mode="nearest")[0, 0, 0].long().numpy()
        assert np.array_equal(got, lpips_ref.nearest_index(n_out, n_in)), (n_out, n_in)


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
    table = getattr(_lib, "LPIPS_SIGNATURES", {})
    assert set(table) == set(decl), "ctypes table out of sync with include/gsr_lpips.h"
    for name, n in decl.items():
        assert len(table[name][1]) == n, f"{name}: {len(table[name][1])} ctypes arguments, the header has {n}"
    assert not set(table) & (set(_lib.SIGNATURES) | set(_lib.GT_SIGNATURES) | set(_lib.EVAL_SIGNATURES)
                             | set(_lib.HIER_BUILD_SIGNATURES) | set(_lib.HIER_MERGE_SIGNATURES))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), f"libgsr_hip.so does not export {name}"
    L = _lib.load()
    assert L.gsr_lpips_tap_scratch_bytes.restype is ctypes.c_size_t
    assert L.gsr_abi_version() == 7 and _lib.ABI_VERSION == 7


def test_native_calls_validate_without_gpu():
    """Argument checks return before any device work."""
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    assert L.gsr_lpips_tap_scratch_bytes(0, 5, 0) == 0 and L.gsr_lpips_tap_scratch_bytes(5, 5, 17) == 0
    # two fp32 sums per row and workgroup, 64 quads of 2x2 pixels per workgroup
    assert L.gsr_lpips_tap_scratch_bytes(5, 7, 0) == 4 * 2 * 1 * 1
    assert L.gsr_lpips_tap_scratch_bytes(106, 159, 5) == 4 * 2 * 6 * math.ceil(53 * 80 / 64)
    one = ctypes.c_void_p(16)  # never dereferenced: the calls fail on their arguments
    assert L.gsr_lpips_prepare(None, None, None, 4, 4, None, None) != 0
    assert b"gsr_lpips_prepare" in L.gsr_last_error()
    assert L.gsr_lpips_prepare(one, one, None, 0, 4, one, None) != 0
    assert L.gsr_lpips_tap(None, None, 64, 4, 4, None, 0, 8, 8, None, None, None, None) != 0
    assert L.gsr_lpips_tap(one, one, 64, 4, 4, None, 17, 8, 8, None, one, one, None) != 0
    assert L.gsr_lpips_tap(one, one, 64, 4, 4, None, 2, 8, 8, None, one, one, None) != 0  # regions, no bits
    assert L.gsr_lpips_tap(one, one, 64, 4, 4, one, 2, 3, 8, None, one, one, None) != 0  # bits plane too small
    assert L.gsr_lpips_tap(one, one, 0, 4, 4, None, 0, 8, 8, None, one, one, None) != 0
    assert b"gsr_lpips_tap" in L.gsr_last_error()
    assert L.gsr_lpips_accumulate(None, None, 1, None, None) != 0
    assert L.gsr_lpips_accumulate(one, one, 18, one, None) != 0


def test_state_dict_key_spellings_and_shape_errors(weights):
    from gs_train.lpips import STAGE_CHANNELS, STAGE_CONVS, LpipsModel
    assert STAGE_CONVS == lpips_ref.STAGE_CONVS and STAGE_CHANNELS == lpips_ref.STAGE_CHANNELS
    vgg, lin = weights
    a = LpipsModel.from_state_dicts(vgg, lin, device="cpu")
    bare = {k[len("features."):]: v for k, v in vgg.items()}
    bare["classifier.0.weight"] = torch.zeros(2, 2)  # ignored
    renamed = {k.replace("lin", "").replace("model.", ""): v for k, v in lin.items()}  # modules/utils.py:22-28
    assert sorted(renamed) == [f"{k}.1.weight" for k in range(5)]
    b = LpipsModel.from_state_dicts(bare, renamed, device="cpu")
    assert [len(s) for s in a.convs] == [2, 2, 3, 3, 3] and [int(v.numel()) for v in a.lins] == [64, 128, 256, 512, 512]
    for sa, sb in zip(a.convs, b.convs):
        for (wa, ba), (wb, bb) in zip(sa, sb):
            assert torch.equal(wa, wb) and torch.equal(ba, bb) and wa.dtype == torch.float32
    assert all(torch.equal(x, y) for x, y in zip(a.lins, b.lins))
    assert torch.equal(a.convs[2][1][0], vgg["features.12.weight"]) and torch.equal(a.lins[3], lin["lin3.model.1.weight"].reshape(512))
    with pytest.raises(KeyError, match="convolution 28"):
        LpipsModel.from_state_dicts({k: v for k, v in vgg.items() if k != "features.28.bias"}, lin, device="cpu")
    with pytest.raises(KeyError, match="linear layer 4"):
        LpipsModel.from_state_dicts(vgg, {k: v for k, v in lin.items() if "lin4" not in k}, device="cpu")
    with pytest.raises(ValueError, match="convolution 5"):
        LpipsModel.from_state_dicts({**vgg, "features.5.weight": torch.zeros(128, 3, 3, 3)}, lin, device="cpu")
    with pytest.raises(ValueError, match="linear layer 1"):
        LpipsModel.from_state_dicts(vgg, {**lin, "lin1.model.1.weight": torch.zeros(1, 64, 1, 1)}, device="cpu")


def test_load_reads_tensor_files_and_the_code_names_no_url(tmp_path, weights):
    from gs_train import lpips as mod
    vgg, lin = weights
    small = {k: v for k, v in vgg.items()}
    torch.save(small, tmp_path / "vgg.pth")
    torch.save(lin, tmp_path / "lin.pth")
    m = mod.LpipsModel.load(tmp_path / "vgg.pth", tmp_path / "lin.pth", device="cpu")
    assert torch.equal(m.convs[0][0][0], vgg["features.0.weight"])
    text = open(mod.__file__).read()
    assert "weights_only=True" in text and not re.search(r"https?:|www\.|load_state_dict_from_url|hub", text)


def test_frame_argument_errors_without_gpu(weights):
    from gs_train.lpips import LpipsModel
    m = LpipsModel.from_state_dicts(*weights, device="cpu")
    img = torch.zeros(3, 16, 20)
    bits = torch.zeros(16, 20, dtype=torch.int16)
    with pytest.raises(ValueError, match="16"):
        m.frame(torch.zeros(3, 15, 20), torch.zeros(3, 15, 20))
    with pytest.raises(ValueError, match="16"):
        m.frame(torch.zeros(3, 20, 8), torch.zeros(3, 20, 8))
    with pytest.raises(ValueError):
        m.frame(img, torch.zeros(3, 16, 21))
    with pytest.raises(ValueError):
        m.frame(img, img, torch.zeros(20, 16))
    with pytest.raises(ValueError):
        m.frame(img, img, None, bits, 17)
    with pytest.raises(ValueError):
        m.frame(img, img, None, None, 2)
    with pytest.raises(ValueError):
        m.frame(img, img, None, bits.to(torch.int32), 2)
    with pytest.raises(RuntimeError):  # valid arguments on the CPU: refused as not on a GPU
        m.frame(img, img, None, bits, 2)


def _totals():
    tot = torch.zeros(10, 6, dtype=torch.float64)
    tot[0] = torch.tensor([2.0 * 25.0 * 100, 2.0 * 0.9 * 100, 2.0 * 0.01 * 100, 2.0 * 0.02 * 100, 200.0, 2.0])
    tot[1] = torch.tensor([30.0 * 40, 0.95 * 40, 0.5 * 40, 0.25 * 40, 40.0, 1.0])
    tot[4] = torch.tensor([21.5 * 10, 0.5 * 10, 0.125 * 10, 0.25 * 10, 10.0, 1.0])
    lp = torch.zeros(10, 2, dtype=torch.float64)
    lp[0] = torch.tensor([0.25 * 200, 200.0])
    lp[1] = torch.tensor([0.125 * 40, 40.0])
    lp[4] = torch.tensor([0.5 * 10, 10.0])
    return tot, lp


def test_evaluator_without_a_model_is_unchanged():
    from gs_train.evaluate import Evaluator
    ev = Evaluator(categories=True)
    assert ev.lpips is None and ev.lpips_totals is None
    tot, _ = _totals()
    res = ev.result(tot)
    assert list(res["whole_image"]) == ["psnr", "ssim", "imae", "irmse", "pixel_count", "image_count"]
    lines = ev.format(tot)
    assert lines[0] == ("Whole Image: PSNR: 25.00000 SSIM: 0.90000 iMAE: 0.01000 iRMSE: 0.02000 "
                        "(pixel-weighted and evaluated on 2 images)")
    assert not any("LPIPS" in ln for ln in lines)


def test_evaluator_with_a_model_reports_the_reference_lines(weights):
    """The reference's format strings (render_hierarchy_final.py:403, 418, 435), field for field."""
    from gs_train.evaluate import Evaluator
    from gs_train.lpips import LpipsModel
    ev = Evaluator(categories=True, lpips=LpipsModel.from_state_dicts(*weights, device="cpu"))
    tot, lp = _totals()
    res = ev.result(tot, lp)
    assert list(res["whole_image"]) == ["psnr", "ssim", "lpips", "imae", "irmse", "pixel_count", "image_count"]
    assert res["whole_image"]["lpips"] == 0.25 and res["depth_near"]["lpips"] == 0.125
    assert res["depth_medium"]["lpips"] is None and res["depth_medium"]["psnr"] is None
    psnr_val, ssim_val, lpips_val, imae_val, irmse_val, count_images = 25.0, 0.9, 0.25, 0.01, 0.02, 2
    whole = (f"Whole Image: PSNR: {psnr_val:.5f} SSIM: {ssim_val:.5f} LPIPS: {lpips_val:.5f} iMAE: {imae_val:.5f} "
             f"iRMSE: {irmse_val:.5f} (pixel-weighted and evaluated on {count_images} images)")
    assert ev.format(tot, lp) == [
        whole,
        "",
        "Depth-Stratified Results:",
        "  Near (0.0-5.0m): PSNR: 30.00000 SSIM: 0.95000 LPIPS: 0.12500 iMAE: 0.50000 iRMSE: 0.25000 "
        "(pixel-weighted and evaluated on 1 instances)",
        "  Medium (5.0-20.0m): No valid pixels found in this depth range.",
        "  Far (20.0m+): No valid pixels found in this depth range.",
        "",
        "Category-Specific Results:",
        "  Category 'sky' : PSNR: 21.50000 SSIM: 0.50000 LPIPS: 0.50000 iMAE: 0.12500 iRMSE: 0.25000 "
        "(pixel-weighted and evaluated on 1 images)",
    ] + [f"  Category '{n}' : Not found or no valid overlap in any evaluated image."
         for n in ["ground", "buildings", "vehicles", "vegetation", "lamposts"]]
    # nothing added yet: every row empty, no device needed
    assert ev.result()["whole_image"]["lpips"] is None
