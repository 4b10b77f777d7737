"""GPU parity on needles, discs, points, reset and faint splats (tests/shape_cases.py).

Every other parity file draws its Gaussians from gs_oracle.synthetic_scene: axis ratios rarely past
5:1, opacities in [0.05, 0.99].  A trained street chunk is needles along kerbs and poles, discs on
facades seen face-on and edge-on, sub-pixel points, whole models at opacity 0.01 after a reset and
rows below 1/255.  Three pieces of this project's own code work hardest on those and the reference
has none of them: the sub-block ellipse cull (ellipse_meets_box, its extents and threshold from the
preprocess), the blend's exponent in the scaled log2 domain, and the backward's replay of it.

(a) One-splat alpha maps.  One Gaussian with colour 1 on black: the image is alpha, final_T is
    1 - alpha and n_contrib is 1 where blended.  Each frame is compared with fp64 evaluated from
    the kernel's own stored record (2D mean, conic, opacity: first checked bit-equal to the
    oracle's), outside and inside the rounding band of the quadratic form (shape_cases.band).  A
    cull that drops a contributing sub-block loses pixels outside the band: a hard failure.
(b) Shape scenes of 3000 rows against the oracle through test_gpu_parity.compare, both binning
    modes (deterministic backward), every claimed population asserted present and barred on its own rows.  Where the oracle
    itself stands further from fp64 than compare's bar (test_oracle.py records its distance per
    tensor and subset in profiles/r12_shape_margins.jsonl), the bar is 4 x the oracle's recorded
    distance from fp64 on the same scene: kernel and oracle are two fp32 evaluations with different
    summation orders.
(c) Backward consistency on the mixed scene: bitwise reproducible in deterministic mode, and the
    segmented backward within (b)'s bars.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import shape_cases as SC
from helpers import decode_state, deterministic, rel_l2, settings, torch_inputs
from test_gpu_parity import GRAD_TOL, NC_TOL, binning_mode, compare, run_hip, run_oracle, upstream_grads

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------
# (a) one-splat alpha maps
# ------------------------------------------------------------------------------------------------
def hip_forward(s):
    """Forward of a one-splat frame through the raw entry point -> (alpha image, decoded state)."""
    import torch
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda:0")
    P = s["means3D"].shape[0]
    inp = torch_inputs(s, dev, use_precomp_colors=True, colors_precomp=np.ones((P, 3), np.float32),
                       requires_grad=False)
    rs = settings(s, dev, 0)
    e = torch.empty(0, device=dev)
    raw = _C.rasterize_gaussians(rs.bg, inp["means3D"], inp["colors_precomp"], inp["opacities"], inp["scales"],
                                 inp["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy,
                                 rs.image_height, rs.image_width, e, 0, rs.campos, False, False, rs.render_indices,
                                 rs.parent_indices, rs.interpolation_weights, rs.num_node_kids, True)
    torch.cuda.synchronize()
    state = decode_state(raw[4], raw[5], raw[6], P, raw[0], s["W"], s["H"])
    return raw[1].cpu().numpy(), raw[3].cpu().numpy(), state


@functools.lru_cache(maxsize=None)
def alpha_frame(f):
    """One frame on the oracle and on the GPU -> (oracle state, kernel image, kernel state, the
    kernel's and the oracle's alpha_map_check)."""
    import gs_oracle as O
    s = SC.single_frame(*f)
    W, H = s["W"], s["H"]
    st = O.forward(s["means3D"], s["opacities"], s["view"], s["proj"], s["campos"], s["bg"], W, H, s["tanfovx"],
                   s["tanfovy"], sh_degree=0, colors_precomp=np.ones((1, 3), np.float32), scales=s["scales"],
                   rotations=s["rotations"])
    img, radii, S = hip_forward(s)
    # the kernel's stored record is the oracle's, bit for bit: fp64 below is evaluated from it
    np.testing.assert_array_equal(radii, st["radii"])
    np.testing.assert_array_equal(S["tiles_touched"], st["tiles_touched"])
    assert st["radii"][0] > 0 and st["tiles_touched"][0] > 0, "the splat is not on screen"
    np.testing.assert_array_equal(S["xy"], st["xy"])
    np.testing.assert_array_equal(S["conic_opacity"], st["conic_opacity"])
    xy, co, r = S["xy"][0], S["conic_opacity"][0], int(radii[0])
    k = SC.alpha_map_check(xy, co, r, W, H, S["n_contrib"] == 1, img[0])
    o = SC.alpha_map_check(xy, co, r, W, H, st["n_contrib"] == 1, st["color"][0])
    SC.record("alpha_map", SC.frame_name(f), kernel_lost=k["lost"], kernel_gained=k["gained"], oracle_lost=o["lost"],
              oracle_gained=o["gained"], n64=k["n64"], in_band=k["in_band"], kernel_must_lost=k["must_lost"],
              kernel_must_gained=k["must_gained"], kernel_alpha_excess=k["alpha_excess"],
              kernel_worst_lost=k["worst_lost"], oracle_worst_lost=o["worst_lost"])
    return st, img, S, k, o


@pytest.mark.parametrize("f", SC.FRAMES, ids=[SC.frame_name(f) for f in SC.FRAMES])
def test_single_splat_alpha_map(f):
    """Per frame, against fp64 from the kernel's own record: every pixel with Q <= tau - 2 gamma is
    blended and none with Q >= tau + 2 gamma (so no contributing sub-block is culled, at any
    orientation, length, centre or opacity); the blended alphas outside the band are fp64's within
    alpha (exp(gamma / 2) - 1 + 2^-21); inside the band, where rounding decides and flips either way
    while a cull error only loses, the kernel loses at most twice the pixels the oracle loses plus
    4 (two fp32 roundings of one quantity; small integers); and the frame's other outputs are
    consistent with an alpha map."""
    st, img, S, k, o = alpha_frame(f)
    nc = S["n_contrib"]
    print(SC.frame_name(f), "kernel", k, "oracle lost/gained", o["lost"], o["gained"])
    assert k["must_lost"] == 0, ("contributing pixels not blended", k)
    assert k["must_gained"] == 0, ("pixels blended that fp64 rejects outside the band", k)
    assert k["alpha_excess"] <= 1.0, k
    assert k["lost"] <= 2 * o["lost"] + 4, (k, o)
    assert nc.max() <= 1
    blended = nc == 1
    np.testing.assert_array_equal(img[1], img[0])
    np.testing.assert_array_equal(img[2], img[0])
    assert not img[0][~blended].any() and (img[0][blended] >= SC.THRESH).all()
    np.testing.assert_array_equal(S["final_T"], np.float32(1) - img[0])
    if f[4] != "thr_dn":
        assert k["n64"] > 0 and blended.any(), "nothing to blend in this frame"


@pytest.mark.parametrize("f", [f for f in SC.FRAMES if f[4] == "thr_dn"], ids=SC.frame_name)
def test_faint_splat_leaves_the_background(f):
    """A splat one float below 1/255 touches tiles and changes nothing: the frame is the background
    exactly and n_contrib is zero everywhere."""
    st, img, S, k, o = alpha_frame(f)
    assert st["tiles_touched"][0] > 0
    assert not img.any() and not S["n_contrib"].any() and (S["final_T"] == 1).all()


# ------------------------------------------------------------------------------------------------
# (b) shape scenes against the oracle
# ------------------------------------------------------------------------------------------------
# px: the needles' and discs' on-screen long sigma in pixels (400-px needles are part (a)'s: the fp32
# gradients of a needle lose a digit for every factor 3 in length, in the oracle and the reference
# alike, and past 200 px a comparison of two fp32 evaluations compares noise)
CASES = [
    dict(name="needles", P=3000, W=256, H=192, deg=3, seed=81, log_scale=-3.0, needle=0.7, px=(8.0, 100.0),
         claims=("thin",)),
    dict(name="discs", P=3000, W=256, H=192, deg=2, seed=82, log_scale=-3.0, disc=0.8, reset=0.7, px=(8.0, 100.0),
         claims=("thin", "reset")),
    dict(name="points_reset", P=3000, W=256, H=192, deg=1, seed=83, log_scale=-3.0, point=0.5, reset=1.0,
         claims=("point", "reset")),
    dict(name="mixed", P=3000, W=256, H=192, deg=3, seed=84, log_scale=-3.0, needle=0.25, disc=0.15, point=0.4,
         reset=0.3, px=(8.0, 100.0), claims=("thin", "point", "reset")),
    dict(name="mixed_faint_640", P=3000, W=640, H=480, deg=3, seed=85, log_scale=-3.0, needle=0.3, disc=0.2, point=0.2,
         reset=0.3, faint=0.1, px=(8.0, 200.0), claims=("thin", "reset", "faint")),
    dict(name="mixed_steep_640", pose="steep", P=3000, W=640, H=480, deg=3, seed=86, log_scale=-3.0, needle=0.25,
         disc=0.15, point=0.4, reset=0.3, px=(8.0, 200.0), claims=("thin", "point", "reset")),
]
BY_NAME = {c["name"]: c for c in CASES}
GRAD_PAIRS = [("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity"), ("shs", "dL_dsh"),
              ("scales", "dL_dscales"), ("rotations", "dL_drotations")]


def shape_bars(c):
    """compare()'s GRAD_TOL, or 4 x the oracle's recorded distance from fp64 on this very scene for
    that tensor and subset where that is larger (profiles/r12_shape_margins.jsonl, kind
    oracle_vs_fp64, case gpu_<name>, written by tools/shape_yardstick.py: fp64 autograd of a
    3000-row frame takes up to half a minute, too long for a test).  The distance is dominated by
    the few longest needles, so it is a property of the scene: the smaller scenes of test_oracle.py,
    which hold the oracle itself in place, stand 2 to 10 times closer to fp64."""
    rec = SC.recorded("oracle_vs_fp64")["gpu_" + c["name"]]
    # n_contrib: NC_TOL is a rate, one pixel in 100 000 whose alpha >= 1/255 or T >= 1e-4 test sits
    # within an exp2 ulp of its threshold.  A 256x192 frame is half that size and cannot express the
    # rate: it gets the one pixel the rate grants a frame of 100 000 (the 640x480 frames keep NC_TOL).  (Seen once: `discs`, pixel
    # (98, 158), the 567th of 1652 positions takes T from 1.18598e-4 to 0.999999e-4 in fp64; the
    # kernel's fp32 product is 1e-4 exactly and blends it, the oracle's is one ulp lower and stops.)
    npix = c["W"] * c["H"]
    bars = dict(nc_bad=max(NC_TOL, 1.5 / npix))  # 1.5: one pixel, clear of the division's rounding
    for hk, ok in GRAD_PAIRS:
        for sub in (None,) + SC.claimed_subsets(c):
            key = ok if sub is None else f"{ok}@{sub}"
            bars["grad_" + hk + ("" if sub is None else "@" + sub)] = max(GRAD_TOL, 4.0 * rec[key])
    return bars


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's scene, upstream gradients, oracle state and gradients and claimed row subsets:
    computed once, shared by the tests (nothing writes to them)."""
    c = BY_NAME[name]
    s = SC.make_scene(c)
    dcol, dinv = upstream_grads(c)
    st, g = run_oracle(s, c, dcol, dinv)
    masks = SC.shape_subsets(s, st)
    SC.assert_shapes_populated(masks, g, c["claims"], s["shape_rows"])
    return s, dcol, dinv, st, g, {k: masks[k] for k in SC.claimed_subsets(c)}


@pytest.mark.parametrize("mode", [0, 1], ids=["local_sort", "global_sort"])
@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_shape_parity_vs_oracle(name, mode):
    """test_parity_vs_oracle's comparison on the shape scenes: radii, tiles_touched, keys, point list
    and ranges bit-exact; image, inverse depth and n_contrib at compare()'s bars; gradients at
    shape_bars over every tensor and over each claimed population's rows alone; every gradient of a
    faint row exactly zero."""
    c = BY_NAME[name]
    s, dcol, dinv, st, g, sub = reference(name)
    # deterministic mode, so that a run's verdict repeats: on needle rows the atomic backward's
    # summation order alone moves a gradient's distance from the oracle by up to 5 x between runs
    # (mixed_faint_640 scales: 0.13 and 0.65), nearer a bar on one day than on another.  The atomic
    # mode's own check is (c), on a scene where it stays under a third of every bar.
    with binning_mode(mode), deterministic():
        h = run_hip(s, c, dcol, dinv)
    if "faint" in sub:
        for hk, _ in GRAD_PAIRS:
            assert not h["grads"][hk].reshape(c["P"], -1)[sub["faint"]].any(), hk
    compare(dict(c, name=f"shape_{name}_{'global' if mode else 'local'}"), st, g, h, global_sort=mode == 1, subsets=sub,
            bars=shape_bars(c))


# ------------------------------------------------------------------------------------------------
# (c) backward consistency
# ------------------------------------------------------------------------------------------------
def test_shape_backward_is_reproducible_and_segments_agree():
    """On the mixed scene: forward + backward twice in deterministic mode give the same bits (the
    replay reproduces the forward's exponent on needles too), and the segmented backward
    (gsr_set_bwd_segment(512); the scene's heaviest tile is past 512 positions) agrees with the
    unsplit one within (b)'s bars."""
    from diff_gaussian_rasterization import _C
    c = BY_NAME["mixed"]
    s, dcol, dinv, st, g, sub = reference("mixed")
    assert int(st["n_contrib"].max()) > 512, "no tile is long enough to be cut into segments"
    prev = _C.set_bwd_segment(0)
    try:
        with deterministic():
            h1 = run_hip(s, c, dcol, dinv)
            h2 = run_hip(s, c, dcol, dinv)
        base = run_hip(s, c, dcol, dinv)
        _C.set_bwd_segment(512)
        seg = run_hip(s, c, dcol, dinv)
    finally:
        _C.set_bwd_segment(prev)
    np.testing.assert_array_equal(h1["color"], h2["color"])
    for k, v in h1["grads"].items():
        np.testing.assert_array_equal(v, h2["grads"][k], err_msg=k)
    np.testing.assert_array_equal(seg["color"], base["color"])
    np.testing.assert_array_equal(seg["state"]["n_contrib"], base["state"]["n_contrib"])
    bars = shape_bars(c)
    compare(dict(c, name="shape_mixed_segmented"), st, g, seg, subsets=sub, bars=bars)
    for hk, _ in GRAD_PAIRS:
        a, b = seg["grads"][hk].reshape(c["P"], -1), base["grads"][hk].reshape(c["P"], -1)
        assert rel_l2(a, b) <= bars["grad_" + hk], hk
        for name, m in sub.items():
            assert rel_l2(a[m], b[m]) <= bars[f"grad_{hk}@{name}"], (hk, name)
