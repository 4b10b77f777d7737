"""CPU tests of the training-view stage: the numpy restatement of the Lanczos resize against Pillow
itself and against the reference's PILtoTorch (tests/golden/views.npz), the coefficient tables the
library makes on the host against the restatement's, target_resolution on hand-worked values, the
linear rule's identity and 2x cases, the mutants of profiles/r22_views_mutation_check.txt, and the C
ABI and the wrappers' refusals without a GPU."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

import views_cases as C
import views_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "views.npz")
LANCZOS = C.lanczos_cases()
EXPAND = C.expand_cases()
_REF = {}


def lanczos_ref(c):
    """The restatement's result of a case, computed once per session and shared."""
    if c["name"] not in _REF:
        _REF[c["name"]] = R.resize_lanczos_ref(c["image"], c["size"])
        _REF[c["name"]].setflags(write=False)
    return _REF[c["name"]]


@pytest.mark.parametrize("c", LANCZOS, ids=[c["name"] for c in LANCZOS])
def test_restatement_equals_pillow(c):
    Image = pytest.importorskip("PIL.Image")
    want = np.array(Image.fromarray(c["image"]).resize(c["size"], Image.LANCZOS))
    got = lanczos_ref(c)
    assert got.shape == want.shape and int((got != want).sum()) == 0


def test_restatement_equals_the_reference_fixture():
    g = np.load(GOLD)
    assert int(g["n"]) == 6 and os.path.getsize(GOLD) < os.path.getsize(os.path.join(REPO, "tests", "golden",
                                                                                      "depth_encode.npz"))
    for k in range(int(g["n"])):
        img, size, out = g[f"in_{k}"], tuple(int(v) for v in g[f"size_{k}"]), g[f"out_{k}"]
        got = R.resize_lanczos_ref(img, size)
        got = got[None] if got.ndim == 2 else got.transpose(2, 0, 1)
        want_u8 = np.rint(out * 255.0).astype(np.uint8)
        assert np.array_equal(got, want_u8), k
        assert np.array_equal(got.astype(np.float32) / np.float32(255.0), out), k  # PILtoTorch's division


def test_cases_reach_both_sides_of_the_clip():
    """The starred cases of the issue's table: the filter's overshoot is clipped at 0 and at 255."""
    for name in ("97x131_to_48x65_c3", "64x64_to_64x32_c3", "64x64_to_32x64_c3", "40x50_to_80x75_c3",
                 "256x300_to_31x299_c3"):
        c = next(c for c in LANCZOS if c["name"] == name)
        img = c["image"].reshape(c["image"].shape[0], c["image"].shape[1], -1)
        w, h = c["size"]
        below = above = 0
        for axis, n in [(axis, n) for axis, n in ((1, w), (0, h)) if img.shape[axis] != n]:
            wide = R._pass(img, axis, n, "", keep_wide=True)  # the pass before its clip
            below, above = below + int((wide < 0).sum()), above + int((wide > 255).sum())
            img = np.clip(wide, 0, 255)
        assert below >= 1 and above >= 1, (name, below, above)
        assert np.array_equal(img.reshape(lanczos_ref(c).shape), lanczos_ref(c))


# ---- the library's host tables --------------------------------------------------------------------

def _plan_tables(in_w, in_h, out_w, out_h, axis):
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    h = ctypes.c_void_p(L.gsr_resize_plan_create(in_w, in_h, out_w, out_h))
    assert h.value
    try:
        info = (ctypes.c_int64 * 5)()
        assert L.gsr_resize_plan_info(h, info, 5) == 0
        n, ksize = (out_w, info[1]) if axis == 0 else (out_h, info[2])
        bounds, coeffs = np.zeros((n, 2), np.int32), np.zeros((n, max(int(ksize), 1)), np.int32)
        p = ctypes.POINTER(ctypes.c_int32)
        rc = L.gsr_resize_plan_tables(h, axis, bounds.ctypes.data_as(p), coeffs.ctypes.data_as(p))
        return rc, list(info), bounds, coeffs
    finally:
        L.gsr_resize_plan_destroy(h)


@pytest.mark.parametrize("sizes", C.LANCZOS_SIZES, ids=[f"{a}_{b}" for a, b in C.LANCZOS_SIZES])
def test_host_tables_equal_the_restatement(sizes):
    """gsr_resize_plan_create makes its tables on the host, as Pillow does (double, libm's sin): they
    equal the restatement's exactly, bounds and 22-bit coefficients, and a skipped axis has none."""
    (H, W), (h, w) = sizes
    for axis, (n_in, n_out) in enumerate(((W, w), (H, h))):
        rc, info, bounds, coeffs = _plan_tables(W, H, w, h, axis)
        assert info[0] == 0  # nothing uploaded: no device was touched
        if n_in == n_out:
            assert rc != 0 and info[1 + axis] == 0
            continue
        ksize, xmin, cnt, coeff = R.lanczos_coeffs(n_in, n_out)
        assert rc == 0 and info[1 + axis] == ksize
        assert np.array_equal(bounds[:, 0], xmin) and np.array_equal(bounds[:, 1], cnt)
        assert np.array_equal(coeffs, coeff)
    taps = {(400, 200): 13, (1000, 125): 49}
    for (n_in, n_out), k in taps.items():  # 6 scale + 1 taps away from the borders
        assert R.lanczos_coeffs(n_in, n_out)[0] == k


# ---- target_resolution ----------------------------------------------------------------------------

def test_target_resolution_hand_worked():
    from gs_train.views import target_resolution as T
    assert T(1536, 1536) == (1536, 1536)                 # -1 under the cap: unchanged
    assert T(1601, 1200) == (1600, 1199)                 # scale 1601/1600: int(1199.25...) = 1199
    assert T(1001, 999, resolution=2) == (500, 500)      # round(500.5) = 500, round(499.5) = 500: ties to even
    assert T(1001, 999, resolution=1) == (1001, 999)
    assert T(4000, 3000, resolution=8) == (500, 375)
    assert T(4000, 3000, resolution=4, resolution_scale=2.0) == (500, 375)
    assert T(4000, 3000, resolution=1000.5) == (1000, 750)  # a float width: int(4000 / (4000 / 1000.5)) = 1000
    assert T(3072, 3072) == (1600, 1600)
    assert T(3072, 3072, resolution_scale=2.0) == (800, 800)
    assert all(isinstance(v, int) for v in T(1001, 999, resolution=2) + T(1601, 1200))


def test_target_resolution_in_the_reference_doubles():
    """reference_floats=True is loadCam:64-81 operation by operation in Python's doubles.  It differs
    from the exact rule by one pixel of width where orig_w / (orig_w / 1600) falls below 1600: 1601 and
    1610 do (1599.9999999999998), 2000 and 3072 do not."""
    from gs_train.views import target_resolution as T
    for w, h in ((1601, 1200), (1610, 1000), (2000, 1500), (3072, 3072), (4001, 17), (1536, 1536)):
        scale = float(w / 1600 if w > 1600 else 1) * float(1.0)
        assert T(w, h, reference_floats=True) == (int(w / scale), int(h / scale))
    assert T(1601, 1200, reference_floats=True) == (1599, 1199) and T(1610, 1000, reference_floats=True)[0] == 1599
    assert T(1610, 1000) == (1600, 993) and T(2000, 1500, reference_floats=True) == T(2000, 1500) == (1600, 1200)
    narrower = [w for w in range(1601, 8000) if T(w, 1000, reference_floats=True)[0] != 1600]
    assert len(narrower) == 464 and all(T(w, 1000)[0] == 1600 for w in range(1601, 8000, 7))
    for args in ((1001, 999, 2), (4000, 3000, 8), (4000, 3000, 1000.5), (1001, 999, 1)):
        assert T(*args) == T(*args, reference_floats=True)
    w, h = 4000, 3000  # the reference's own lines for a float width
    scale = float(w / 1000.5) * float(1.0)
    assert T(w, h, 1000.5, reference_floats=True) == (int(w / scale), int(h / scale))


# ---- the linear rule ------------------------------------------------------------------------------

def test_linear_rule_is_the_identity_at_equal_sizes():
    rng = np.random.default_rng(3)
    S = rng.normal(size=(13, 17)).astype(np.float32)
    S[2, 3] = -0.0
    out = R.resize_linear_ref(S, (17, 13))
    assert out.dtype == np.float32 and np.array_equal(out, S)


def test_linear_rule_at_2x_is_the_2x2_mean_to_one_rounding():
    rng = np.random.default_rng(4)
    S = rng.uniform(0.0, 4.0, (24, 30)).astype(np.float32)
    out = R.resize_linear_ref(S, (15, 12))
    ix, fx = R.linear_taps(30, 15)
    assert np.array_equal(ix, 2 * np.arange(15)) and np.all(fx == 0.5)  # every tap halfway between two samples
    mean = S.astype(np.float64).reshape(12, 2, 15, 2).mean(axis=(1, 3))
    # the products by 0.5 are exact, so three float32 sums round: at most 1.5 ulp of the result, and
    # the result is below 4: ulp <= 2^-22
    assert np.abs(out.astype(np.float64) - mean).max() <= 1.5 * 2.0 ** -22
    up = R.resize_linear_ref(S, (60, 48))  # borders replicate: the corners are the source's corners
    assert up[0, 0] == S[0, 0] and up[-1, -1] == S[-1, -1]


# ---- the expansion's restatement ------------------------------------------------------------------

@pytest.mark.parametrize("c", EXPAND, ids=[c["name"] for c in EXPAND])
def test_expand_restatement_against_torch(c):
    """Without depth the restatement is torch's own CPU arithmetic of PILtoTorch and Camera.__init__;
    with depth its shapes, its clip and its mask follow the rule."""
    import torch
    want = R.expand_ref(**{k: c[k] for k in ("image", "mask", "u16", "scale", "offset", "size", "depth_only",
                                            "test_half", "depth_valid")})
    w, h = c["size"]
    alpha = torch.ones(1, h, w) if c["mask"] is None else (torch.from_numpy(c["mask"]) / 255.0)[None]
    if c["test_half"] == "left":
        alpha[..., :w // 2] = 0
    elif c["test_half"] == "right":
        alpha[..., w // 2:] = 0
    if c["depth_only"]:
        img = torch.zeros(3, h, w)
    else:
        img = (torch.from_numpy(c["image"]) / 255.0).permute(2, 0, 1).clamp(0.0, 1.0) * alpha
    assert np.array_equal(want["original_image"], img.numpy()) and want["original_image"].dtype == np.float32
    assert np.array_equal(want["alpha_mask"], alpha.numpy())
    if c["u16"] is None or not c["scale"] > 0:
        assert want["invdepthmap"] is None and want["depth_mask"] is None
        return
    d = want["invdepthmap"]
    assert d.shape == (1, h, w) and d.dtype == np.float32 and d.min() >= 0
    if c["u16"].shape == (h, w):  # equal sizes: the affine map and the clip alone
        s = torch.from_numpy(c["u16"].astype(np.float32)) / 65536.0 * c["scale"] + c["offset"]
        assert np.array_equal(d[0], s.clamp_min(0.0).numpy())
    hit = want["alpha_mask"] * (d != 0) if c["depth_valid"] == "alpha_and_hit" else want["alpha_mask"]
    assert np.array_equal(want["depth_mask"], hit.astype(np.float32))


# ---- the mutants (profiles/r22_views_mutation_check.txt) -------------------------------------------

LANCZOS_MUTANTS = ["round_neg", "no_half", "vertical_first", "no_u8_between"]


@pytest.mark.parametrize("mutant", LANCZOS_MUTANTS)
def test_lanczos_mutants_are_caught(mutant):
    caught = [c["name"] for c in LANCZOS[:24]
              if not np.array_equal(R.resize_lanczos_ref(c["image"], c["size"], mutant=mutant), lanczos_ref(c))]
    assert len(caught) >= 4, (mutant, caught)


def test_xmin_without_the_half_changes_the_table_and_not_the_image():
    """int(center - support) instead of int(center - support + 0.5) starts a window at most one
    sample earlier, and that sample's argument is below -3, where the filter is exactly 0: the image
    is the same (an equivalent mutant there), the tap counts the library reports are not."""
    changed = 0
    for (H, W), (h, w) in C.LANCZOS_SIZES[:12]:
        for n_in, n_out in ((W, w), (H, h)):
            if n_in == n_out:
                continue
            _, xmin, cnt, coeff = R.lanczos_coeffs(n_in, n_out)
            _, xmin_m, cnt_m, coeff_m = R.lanczos_coeffs(n_in, n_out, mutant="xmin_trunc")
            for xx in np.nonzero(xmin_m != xmin)[0]:
                assert xmin_m[xx] == xmin[xx] - 1 and coeff_m[xx, 0] == 0
                assert np.array_equal(coeff_m[xx, 1:cnt_m[xx]], coeff[xx, :cnt[xx]])
                changed += 1
    assert changed > 0


def test_expand_mutants_are_caught():
    key = ("image", "mask", "u16", "scale", "offset", "size", "depth_only", "test_half", "depth_valid")
    caught = {"reciprocal": 0, "clip_first": 0}
    for c in EXPAND:
        want = R.expand_ref(**{k: c[k] for k in key})
        for m in caught:
            got = R.expand_ref(mutant=m, **{k: c[k] for k in key})
            same = all((want[p] is None and got[p] is None) or np.array_equal(want[p], got[p]) for p in want)
            caught[m] += not same
    assert caught["reciprocal"] >= 4 and caught["clip_first"] >= 2, caught


# ---- the C ABI and the wrappers without a GPU ------------------------------------------------------

def test_lib_declares_and_exports_the_header_entry_points():
    from diff_gaussian_rasterization import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gsr_views.h")).read(), flags=re.S)
    decl = {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\b(gsr_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}
    assert set(decl) == {"gsr_resize_plan_create", "gsr_resize_plan_destroy", "gsr_resize_plan_info",
                         "gsr_resize_plan_tables", "gsr_resize_scratch_bytes", "gsr_resize_lanczos_u8",
                         "gsr_view_expand"}
    table = _lib.VIEWS_SIGNATURES
    assert set(table) == set(decl)
    for name, n in decl.items():
        assert len(table[name][1]) == n, name
    others = (set(_lib.SIGNATURES) | set(_lib.GT_SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.HIER_BUILD_SIGNATURES)
              | set(_lib.HIER_MERGE_SIGNATURES) | set(_lib.LPIPS_SIGNATURES) | set(_lib.MODEL_INIT_SIGNATURES)
              | set(_lib.LIDAR_SIGNATURES) | set(_lib.MESH_DEPTH_SIGNATURES) | set(_lib.CHUNKER_SIGNATURES))
    assert not set(table) & others
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in decl:
        assert hasattr(raw, name)
    assert _lib.load().gsr_abi_version() == _lib.ABI_VERSION == 7  # new entry points only


def test_calls_validate_without_gpu():
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    for bad in ((0, 4, 4, 4), (4, 4, 4, 0), (40000, 4, 4, 4), (4, -1, 4, 4)):
        assert not L.gsr_resize_plan_create(*bad)
        assert b"gsr_resize_plan_create" in L.gsr_last_error()
    h = ctypes.c_void_p(L.gsr_resize_plan_create(64, 48, 20, 15))
    try:
        assert L.gsr_resize_scratch_bytes(h, 3) == 20 * 48 * 3 and L.gsr_resize_scratch_bytes(h, 1) == 20 * 48
        assert L.gsr_resize_scratch_bytes(h, 4) == 0 and L.gsr_resize_scratch_bytes(None, 3) == 0
        assert L.gsr_resize_lanczos_u8(h, None, 4, None, None, None) != 0
        assert b"premultiplies" in L.gsr_last_error()  # the 4-channel refusal says why
        assert L.gsr_resize_lanczos_u8(h, None, 2, None, None, None) != 0
        assert L.gsr_resize_lanczos_u8(h, None, 3, None, None, None) != 0  # NULL pointers
        assert L.gsr_resize_lanczos_u8(None, None, 3, None, None, None) != 0
        assert L.gsr_resize_plan_tables(h, 2, None, None) != 0
    finally:
        L.gsr_resize_plan_destroy(h)
    L.gsr_resize_plan_destroy(None)
    h = ctypes.c_void_p(L.gsr_resize_plan_create(64, 48, 64, 15))  # one pass: no scratch
    assert L.gsr_resize_scratch_bytes(h, 3) == 0
    L.gsr_resize_plan_destroy(h)
    ok = dict(W=4, H=4, rgb=None, mask=None, zero_half=0, depth=None, dW=0, dH=0, scale=0.0, offset=0.0, depth_valid=0,
              image=16, alpha=16, invdepth=None, depth_mask=None, stream=None)
    for kw in (dict(W=0), dict(H=40000), dict(zero_half=3), dict(depth_valid=2), dict(image=None), dict(alpha=None),
               dict(image=20), dict(alpha=8), dict(invdepth=16), dict(depth=2, dW=4, dH=4), dict(rgb=2), dict(mask=1),
               dict(depth=2, dW=0, dH=4, invdepth=16, depth_mask=16),
               dict(depth=2, dW=4, dH=4, invdepth=16, depth_mask=16, scale=float("nan"))):
        assert L.gsr_view_expand(*dict(ok, **kw).values()) != 0, kw
        assert b"gsr_view_expand" in L.gsr_last_error()


def test_wrappers_check_their_arguments_without_gpu():
    import torch
    from gs_train import views as V
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        V.ResizePlan(8, 8, 4, 4).resize(torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="premultiplies"):
        V.resize_lanczos(np.zeros((8, 8, 4), np.uint8), (4, 4), device="cpu")
    with pytest.raises(ValueError, match="32768"):
        V.ResizePlan(8, 8, 0, 4)
    store = V.ViewStore(device="cpu")
    with pytest.raises(ValueError, match="premultiplies"):
        store.add(image=np.zeros((8, 8, 4), np.uint8))
    for bad in (np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8), np.float32), np.zeros((8, 8), np.uint16),
                torch.zeros(8, 8, 1, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="single-channel"):
            store.add(image=np.zeros((8, 8, 3), np.uint8), mask=bad)
    with pytest.raises(ValueError, match="65535"):
        store.add(image=np.zeros((8, 8, 3), np.uint8), invdepth_u16=np.full((8, 8), 70000), scale=1.0)
    with pytest.raises(ValueError, match="test_half"):
        store.add(image=np.zeros((8, 8, 3), np.uint8), test_half="top")
    with pytest.raises(ValueError, match="depth_valid"):
        store.add(image=np.zeros((8, 8, 3), np.uint8), depth_valid="hit")
    with pytest.raises(ValueError, match="needs an image"):
        store.add()
    assert len(store) == 0
    # the compact store and its accounting need no kernel
    k = store.add(image=np.zeros((6, 10, 3), np.uint8), mask=np.zeros((6, 10), np.uint8),
                  invdepth_u16=np.zeros((12, 20), np.int64), scale=0.5)
    j = store.add(invdepth_u16=np.zeros((6, 10), np.uint16), scale=0.0, depth_only=True)
    assert (k, j) == (0, 1) and len(store.gts) == 2 and store.depth_only == [False, True]
    nb = store.nbytes()
    assert nb["compact"] == 6 * 10 * 4 + 12 * 20 * 2 + 6 * 10 * 2
    assert nb["expanded"] == 6 * 240 + 4 * 240 and nb["planes"] == 2 * 6 * 240 and nb["views"] == 2
    with pytest.raises(IndexError):
        store.gts[2]
