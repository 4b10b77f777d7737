"""CPU tests of the oracle: pinned against the reference's own helpers (golden fixtures made by
tests/golden/make_golden.py from /root/reference) and against an independent fp64 autograd
formulation (oracle/dense_torch.py) of the same renderer."""
from __future__ import annotations

import os

import numpy as np
import pytest

import dense_torch as DT
import gs_oracle as O
from helpers import rel_l2

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_sh_matches_reference_eval_sh():
    g = np.load(os.path.join(GOLD, "sh_eval.npz"))
    for deg in range(4):
        rgb, clamped = O.eval_sh(deg, g["sh"], g["dirs"])
        np.testing.assert_array_equal(rgb, g[f"rgb_deg{deg}"])  # bit-exact
        np.testing.assert_array_equal(clamped, (g[f"eval_deg{deg}"] + 0.5) < 0)


def test_covariance_matches_reference_get_covariance():
    c = np.load(os.path.join(GOLD, "covariance.npz"))
    for mod in (1.0, 0.5, 2.0):
        np.testing.assert_array_equal(O.cov3d(c["scales"], c["rot_normalized"], mod), c[f"cov_mod{mod}"])


def test_camera_matrices_match_reference():
    cams = np.load(os.path.join(GOLD, "cameras.npz"))
    for i in range(int(cams["n"])):
        k = lambda n: cams[f"cam{i}_{n}"]
        v, p, cp, tx, ty = O.camera_from(int(k("W")), int(k("H")), k("R"), k("T"), float(k("FoVx")),
                                         float(k("FoVy")), float(k("primx")), float(k("primy")))
        np.testing.assert_array_equal(v, k("viewmatrix"))
        np.testing.assert_array_equal(p, k("projmatrix"))
        np.testing.assert_allclose(cp, k("campos"), atol=1e-6)
        assert tx == pytest.approx(float(k("tanfovx")), abs=0)
        assert ty == pytest.approx(float(k("tanfovy")), abs=0)


def _scene(P, W, H, seed, deg, log_scale=-3.0, spread=0.95, **kw):
    s = O.synthetic_scene(P, W, H, seed=seed, sh_degree=3, log_scale_mean=log_scale, **kw)
    if spread != 0.95:  # push some means outside the 1.3*tanfov clamp
        rng = np.random.default_rng(seed + 7)
        m = s["means3D"]
        m[:, 0] = rng.uniform(-spread, spread, P) * s["tanfovx"] * m[:, 2]
        m[:, 1] = rng.uniform(-spread, spread, P) * s["tanfovy"] * m[:, 2]
    return s


def _fwd(s, W, H, deg, **kw):
    return O.forward(s["means3D"], s["opacities"], s["view"], s["proj"], s["campos"], s["bg"], W, H, s["tanfovx"],
                     s["tanfovy"], sh_degree=deg, **kw)


DENSE_CASES = [
    dict(P=300, W=64, H=48, seed=3, deg=3, log_scale=-2.5),
    dict(P=600, W=70, H=50, seed=4, deg=1, log_scale=-2.7),
    dict(P=400, W=64, H=64, seed=5, deg=2, log_scale=-2.6, spread=1.8),   # means out to 1.8*tanfov, but none
    # of the rows past the 1.3*tanfov clamp reaches a pixel (posed_cases.subsets: 0 `beyond` rows): the clamp's
    # backward is carried by POSED_DENSE_CASES' steep_all below
    dict(P=400, W=80, H=48, seed=6, deg=0, log_scale=-2.4, mod=1.6),      # scale_modifier != 1
    dict(P=400, W=64, H=48, seed=8, deg=3, log_scale=-2.5, primx=0.35, primy=0.6),
]


@pytest.mark.parametrize("c", DENSE_CASES)
def test_oracle_backward_matches_fp64_autograd(c):
    W, H, deg = c["W"], c["H"], c["deg"]
    kw = {k: c[k] for k in ("primx", "primy") if k in c}
    s = _scene(c["P"], W, H, c["seed"], deg, c["log_scale"], c.get("spread", 0.95), **kw)
    st = _fwd(s, W, H, deg, shs=s["shs"], scales=s["scales"], rotations=s["rotations"],
              scale_modifier=c.get("mod", 1.0))
    rng = np.random.default_rng(0)
    gc = rng.normal(size=(3, H, W))
    gd = rng.normal(size=(1, H, W))
    b = O.backward(st, gc, gd, true_scale_grad=True)  # fp64 autograd gives the exact derivative
    d = DT.dense_grads(st, gc, gd)
    # upstream's convention (the default): dL/d(mod * s) reported as dL/ds
    bu = O.backward(st, gc, gd)
    assert rel_l2(bu["dL_dscales"] * np.float32(c.get("mod", 1.0)), b["dL_dscales"]) < 1e-6
    assert rel_l2(st["color"], d["color"]) < 1e-5
    assert rel_l2(st["invdepth"], d["invdepth"]) < 1e-5
    for dk, ok in [("dL_dmeans3D", "dL_dmeans3D"), ("dL_dmeans2D", "dL_dmeans2D"), ("dL_dopacities", "dL_dopacity"),
                   ("dL_dshs", "dL_dsh"), ("dL_dscales", "dL_dscales"), ("dL_drotations", "dL_drotations")]:
        assert rel_l2(b[ok].reshape(d[dk].shape), d[dk]) < 5e-5, dk


FP64_PAIRS = [("dL_dmeans3D", "dL_dmeans3D"), ("dL_dmeans2D", "dL_dmeans2D"), ("dL_dopacities", "dL_dopacity"),
              ("dL_dshs", "dL_dsh"), ("dL_dscales", "dL_dscales"), ("dL_drotations", "dL_drotations")]

# Posed cameras and the clamp populations (tests/posed_cases.py): the identity camera of the cases
# above hides the view rotation, the translation row, campos and the off-diagonal projection entries
POSED_DENSE_CASES = [
    dict(name="steep_plain", pose="steep", P=450, W=64, H=48, seed=31, deg=3, log_scale=-2.5),
    # splats of a pixel or more and a larger opaque share: a 500-row scene then holds 20 capped rows
    dict(name="steep_all", pose="steep", P=500, W=70, H=50, seed=34, deg=2, log_scale=-1.5, primx=0.35, primy=0.6,
         edge=0.3, opaque=0.4, dark=2.0),
    dict(name="cam1", pose="cam1", P=400, W=96, H=64, seed=33, deg=3, log_scale=-2.5),
    dict(name="steep_modifier", pose="steep", P=400, W=64, H=48, seed=34, deg=1, log_scale=-2.6, mod=1.6),
]


def _posed(c):
    import posed_cases as PC
    s = PC.make_scene(c)
    st = _fwd(s, c["W"], c["H"], c["deg"], shs=s["shs"], scales=s["scales"], rotations=s["rotations"],
              scale_modifier=c.get("mod", 1.0))
    return s, st


@pytest.mark.parametrize("c", POSED_DENSE_CASES, ids=[c["name"] for c in POSED_DENSE_CASES])
def test_oracle_backward_matches_fp64_autograd_posed(c):
    """The oracle against fp64 autograd under posed cameras, with the 1.3 * tanfov clamp, the 0.99
    alpha cap and the SH colour clamp populated; the bars of the identity-camera test, applied to
    every tensor and again to the rows of each population alone (posed_cases.subsets)."""
    import posed_cases as PC
    W, H = c["W"], c["H"]
    s, st = _posed(c)
    rng = np.random.default_rng(0)
    gc = rng.normal(size=(3, H, W))
    gd = rng.normal(size=(1, H, W))
    b = O.backward(st, gc, gd, true_scale_grad=True)
    d = DT.dense_grads(st, gc, gd)
    masks = PC.subsets(s, st)
    PC.assert_populated(masks, b, PC.claims(c))
    assert int((st["radii"] > 0).sum()) > 0.5 * c["P"]
    assert rel_l2(st["color"], d["color"]) < 1e-5
    assert rel_l2(st["invdepth"], d["invdepth"]) < 1e-5
    for dk, ok in FP64_PAIRS:
        got, ref = b[ok].reshape(d[dk].shape), d[dk]
        assert rel_l2(got, ref) < 5e-5, dk
        for name in PC.claimed_subsets(c):
            m = masks[name]
            assert rel_l2(got[m], ref[m]) < 5e-5, (dk, name, int(m.sum()))


# Needles, discs, points, reset and faint splats (tests/shape_cases.py), identity and steep pose.
# px: the needles' and discs' on-screen long sigma, log-uniform in pixels; the distance from fp64 grows with
# its square (needles to 120 / 200 / 400 px: dL_dmeans3D 2e-2 / 3e-2 / 1e-1) and is carried by a scene's few
# longest needles.  These cases hold the oracle in place on each population; the GPU bars of
# test_gpu_shapes.py are stated against its distance on the GPU scenes themselves (tools/shape_yardstick.py).
SHAPE_DENSE_CASES = [
    dict(name="needles", P=400, W=96, H=64, seed=71, deg=3, log_scale=-2.5, needle=0.7, px=(8.0, 100.0),
         claims=("thin",)),
    dict(name="discs_steep", pose="steep", P=400, W=160, H=120, seed=72, deg=2, log_scale=-2.5, disc=0.8,
         reset=0.7, px=(8.0, 100.0), claims=("thin", "reset")),   # unreset, the face-on discs hide most rows
    dict(name="points_reset_steep", pose="steep", P=500, W=96, H=64, seed=73, deg=1, log_scale=-2.5, point=0.5,
         reset=1.0, claims=("point", "reset")),
    dict(name="mixed_faint", P=500, W=160, H=120, seed=74, deg=3, log_scale=-2.5, needle=0.3, disc=0.2, point=0.2,
         reset=0.3, faint=0.15, px=(8.0, 200.0), claims=("thin", "reset", "faint")),
    dict(name="mixed_steep", pose="steep", P=500, W=160, H=120, seed=75, deg=3, log_scale=-3.0, needle=0.25, disc=0.15,
         point=0.55, reset=0.3, px=(8.0, 100.0), claims=("thin", "point", "reset")),
    dict(name="mixed_steep_long", pose="steep", P=500, W=160, H=120, seed=76, deg=3, log_scale=-3.0, needle=0.25,
         disc=0.15, point=0.55, reset=0.3, px=(8.0, 200.0), claims=("thin", "point", "reset")),
]
DENSE_BAR = 5e-5  # the bar of the cases above


@pytest.mark.parametrize("c", SHAPE_DENSE_CASES, ids=[c["name"] for c in SHAPE_DENSE_CASES])
def test_oracle_backward_matches_fp64_autograd_shapes(c):
    """The oracle against fp64 autograd on needles, discs, points, reset and faint splats, over every
    tensor and over the rows of each claimed population alone.  Gradients of near-singular 2D
    covariances are ill-conditioned in fp32 (the reference's arithmetic shares that), so where the
    5e-5 bar of the cases above does not hold the oracle is held to twice its own recorded distance
    (profiles/r12_shape_margins.jsonl, kind oracle_vs_fp64; written by this test when
    GSR_SHAPE_RECORD is set), so that a later change to the oracle cannot drift."""
    import shape_cases as SC
    W, H = c["W"], c["H"]
    s = SC.make_scene(c)
    st = _fwd(s, W, H, c["deg"], shs=s["shs"], scales=s["scales"], rotations=s["rotations"])
    rng = np.random.default_rng(0)
    gc = rng.normal(size=(3, H, W))
    gd = rng.normal(size=(1, H, W))
    b = O.backward(st, gc, gd, true_scale_grad=True)
    d = DT.dense_grads(st, gc, gd)
    masks = SC.shape_subsets(s, st)
    SC.assert_shapes_populated(masks, b, c["claims"], s["shape_rows"])
    err = dict(color=rel_l2(st["color"], d["color"]), invdepth=rel_l2(st["invdepth"], d["invdepth"]))
    for dk, ok in FP64_PAIRS:
        got, ref = b[ok].reshape(d[dk].shape), d[dk]
        err[ok] = rel_l2(got, ref)
        for name in SC.claimed_subsets(c):
            err[f"{ok}@{name}"] = rel_l2(got[masks[name]], ref[masks[name]])
    if "faint" in c["claims"]:
        for dk, ok in FP64_PAIRS:
            assert not b[ok].reshape(c["P"], -1)[masks["faint"]].any(), ok
            assert not d[dk].reshape(c["P"], -1)[masks["faint"]].any(), dk
    print(c["name"], {k: f"{v:.2e}" for k, v in err.items()})
    SC.record("oracle_vs_fp64", c["name"], **err)
    rec = SC.recorded("oracle_vs_fp64")[c["name"]]
    for k, v in err.items():
        assert v <= max(1e-5 if k in ("color", "invdepth") else DENSE_BAR, 2.0 * rec[k]), (k, v, rec[k])


def _band_frames():
    import shape_cases as SC
    return [f for f in SC.FRAMES if f[0] == "needle" and f[4] in ("o99", "o01")]


def test_oracle_blend_decision_matches_fp64_outside_the_rounding_band():
    """Single needles (sigma 10, 100, 400 px; 0, 1, 45, 89, 90 degrees; opacity 0.99 and 0.01; on and
    off screen): the oracle blends every pixel fp64 blends and no other, except inside the band
    |Q - tau| <= 2 gamma, where fp32 rounding of the quadratic form decides (shape_cases.band); its
    alpha is fp64's within the band's bound; and the band holds at most 5 % of the fp64-blended
    pixels of every frame whose needle is centred on screen at opacity 0.99.  (The band is a strip along
    the alpha = 1/255 contour.  A needle centred 200 px outside shows its tail alone and one at opacity
    0.01 blends a core 1.5 px wide, so most of their pixels lie near the contour: 15 to 20 % in the
    band at sigma 400.  Those frames are held to the decision and alpha checks alone.)
    The GPU alpha-map test applies the same check to the kernels."""
    import shape_cases as SC
    frames = _band_frames()
    assert len(frames) >= 30
    worst_share = 0.0
    for f in frames:
        s = SC.single_frame(*f)
        st = O.forward(s["means3D"], s["opacities"], s["view"], s["proj"], s["campos"], s["bg"], s["W"], s["H"],
                       s["tanfovx"], s["tanfovy"], sh_degree=0, colors_precomp=np.ones((1, 3), np.float32),
                       scales=s["scales"], rotations=s["rotations"])
        r = SC.alpha_map_check(st["xy"][0], st["conic_opacity"][0], int(st["radii"][0]), s["W"], s["H"],
                               st["n_contrib"] > 0, st["color"][0])
        SC.record("oracle_band", SC.frame_name(f), **r)
        assert r["n64"] > 0, f
        assert r["must_lost"] == 0 and r["must_gained"] == 0, (f, r)
        assert r["alpha_excess"] <= 1.0, (f, r)
        if f[3] != "off" and f[4] == "o99":
            assert r["in_band"] <= 0.05 * r["n64"], (f, r)
            worst_share = max(worst_share, r["in_band"] / r["n64"])
    print("largest band share", worst_share)


def test_alpha_map_frames_cover_the_claimed_shapes():
    """Conditions on the inputs: about 60 frames; needles and edge-on discs are thin on screen
    (eigenvalue ratio of the 2D covariance >= 100) at long sigmas within 5 % of 10, 100 and 400 px;
    points carry the 0.3 low-pass term alone (off-diagonal below 1e-10); the `pixel` centres are pixel
    centres exactly and the `sbrow` centres lie on a row y = 4k."""
    import shape_cases as SC
    assert 55 <= len(SC.FRAMES) <= 70
    for f in SC.FRAMES:
        if f[3] == "off":
            continue  # past the 1.3 * tanfov clamp the projected axes stretch
        s = SC.single_frame(*f)
        st = O.forward(s["means3D"], s["opacities"], s["view"], s["proj"], s["campos"], s["bg"], s["W"], s["H"],
                       s["tanfovx"], s["tanfovy"], sh_degree=0, colors_precomp=np.ones((1, 3), np.float32),
                       scales=s["scales"], rotations=s["rotations"])
        ratio, sigma = SC.conic_axes(st["conic_opacity"])
        if f[0] in ("needle", "edge_disc"):
            assert ratio[0] >= 100.0 and abs(sigma[0] / f[1] - 1.0) < 0.05, (f, ratio, sigma)
        if f[0] == "point":
            inv = np.float32(1) / np.float32(0.3)
            assert abs(st["conic_opacity"][0, 0] / inv - 1) < 1e-6 and abs(st["conic_opacity"][0, 1]) < 1e-10 and \
                st["radii"][0] == 3
        if f[3] == "pixel":
            assert np.array_equal(st["xy"][0], np.rint(st["xy"][0])), (f, st["xy"])
        if f[3] == "sbrow":
            assert st["xy"][0, 1] % 4 == 0, (f, st["xy"])


def test_oracle_precomputed_paths_match_fp64_autograd():
    _precomputed_paths_match_fp64_autograd(posed=False)


def test_oracle_precomputed_paths_match_fp64_autograd_posed():
    _precomputed_paths_match_fp64_autograd(posed=True)


def _precomputed_paths_match_fp64_autograd(posed):
    W, H = 64, 48
    if posed:  # steep camera, rows past the 1.3 * tanfov clamp and capped alphas
        import posed_cases as PC
        s = PC.make_scene(dict(pose="steep", P=400, W=W, H=H, seed=9, log_scale=-2.5, edge=0.3, opaque=0.2))
    else:
        s = _scene(400, W, H, 9, 3, -2.5)
    colors =np.random.default_rng(1).uniform(0, 1, (400, 3)).astype(np.float32)
    cov = O.cov3d(s["scales"], s["rotations"])
    st = _fwd(s, W, H, 3, colors_precomp=colors, cov3D_precomp=cov)
    rng = np.random.default_rng(2)
    gc, gd = rng.normal(size=(3, H, W)), rng.normal(size=(1, H, W))
    b = O.backward(st, gc, gd)
    d = DT.dense_grads(st, gc, gd)
    for dk, ok in [("dL_dmeans3D", "dL_dmeans3D"), ("dL_dopacities", "dL_dopacity"), ("dL_dcolors", "dL_dcolors"),
                   ("dL_dcov3D", "dL_dcov3D")]:
        assert rel_l2(b[ok].reshape(d[dk].shape), d[dk]) < 5e-5, dk


def test_cross_path_identity_in_oracle():
    """(shs, scales, rotations) == (colors_precomp from eval_sh, cov3D_precomp from cov3d) exactly."""
    W, H = 96, 64
    s = _scene(1500, W, H, 10, 3)
    a = _fwd(s, W, H, 3, shs=s["shs"], scales=s["scales"], rotations=s["rotations"])
    d = s["means3D"] - s["campos"]
    dn = (d / np.sqrt((d.astype(np.float32) ** 2).sum(1, keepdims=True))).astype(np.float32)
    # direction normalisation differs in rounding between numpy and C: compare images, not bits
    rgb, _ = O.eval_sh(3, s["shs"], dn)
    b = _fwd(s, W, H, 3, colors_precomp=rgb, cov3D_precomp=O.cov3d(s["scales"], s["rotations"]))
    np.testing.assert_array_equal(a["radii"], b["radii"])
    np.testing.assert_array_equal(a["point_list"], b["point_list"])
    assert np.abs(a["color"] - b["color"]).max() < 1e-5


def test_binning_invariants():
    W, H = 200, 120
    s = _scene(3000, W, H, 11, 3, -3.2)
    st = _fwd(s, W, H, 3, shs=s["shs"], scales=s["scales"], rotations=s["rotations"])
    keys, pl, rng_ = st["keys"], st["point_list"], st["ranges"]
    assert st["K"] == int(st["tiles_touched"].sum())
    assert np.all(keys[1:] >= keys[:-1])
    tiles = (keys >> np.uint64(32)).astype(np.int64)
    dbits = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    np.testing.assert_array_equal(dbits, st["depths"][pl].view(np.uint32))
    for t in np.unique(tiles):
        lo, hi = rng_[t]
        assert np.all(tiles[lo:hi] == t)
    # stable: equal keys keep Gaussian-index order
    same = keys[1:] == keys[:-1]
    assert np.all(pl[1:][same] > pl[:-1][same])
    # n_contrib never exceeds the tile's list length
    gx = (W + 15) // 16
    for y in range(0, H, 7):
        for x in range(0, W, 7):
            t = (y // 16) * gx + x // 16
            assert st["n_contrib"][y, x] <= rng_[t, 1] - rng_[t, 0]


def test_empty_and_culled_inputs():
    W, H = 40, 30
    s = _scene(20, W, H, 12, 0)
    s["means3D"][:, 2] = -1.0
    st = _fwd(s, W, H, 0, shs=s["shs"], scales=s["scales"], rotations=s["rotations"])
    assert st["K"] == 0 and np.all(st["radii"] == 0)
    np.testing.assert_allclose(st["color"], np.broadcast_to(s["bg"][:, None, None], (3, H, W)))
    b = O.backward(st, np.ones((3, H, W)), np.ones((1, H, W)))
    assert np.all(b["dL_dmeans3D"] == 0)
    assert not O.mark_visible(s["means3D"], s["view"], s["proj"]).any()


def test_render_post_interpolation_fixture():
    """Pins the hierarchy LOD interpolation render_post performs before rasterizing
    (gaussian_renderer/__init__.py:200-243) -- the input contract of SURVEY 8(f) row 3 -- and the
    oracle restatement the fused kernel is tested against (oracle/hier_ref.py)."""
    import hier_ref
    f = np.load(os.path.join(GOLD, "render_post.npz"))
    o = hier_ref.interpolate_cut(f["xyz"], f["scaling"], f["rotation"], f["opacity"], f["features"],
                                 f["render_indices"], f["parent_indices"], f["interpolation_weights"], int(f["skybox"]))
    for k in ("means3D", "scales", "rotations", "opacities", "shs"):
        np.testing.assert_allclose(o[k], f["out_" + k], rtol=0, atol=1e-6, err_msg=k)


def test_knn_oracle_matches_float64_brute_force():
    """The distCUDA2 restatement (parity unpinned: simple-knn is not vendored) against an fp64
    numpy brute force, plus its small-N conventions (missing neighbours are FLT_MAX)."""
    rng = np.random.default_rng(3)
    p = rng.normal(size=(1500, 3)).astype(np.float32)
    p[100:110] = p[50]  # duplicates count as distance 0
    got = O.knn_mean_dist2(p)
    d = ((p[None].astype(np.float64) - p[:, None]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    ref = np.sort(d, 1)[:, :3].mean(1)
    assert np.abs(got - ref).max() <= 1e-6 * ref.max()
    assert (got[100:110] == 0).all()
    flt_max = np.finfo(np.float32).max
    assert np.all(O.knn_mean_dist2(np.zeros((3, 3))) == np.float32((0 + 0 + flt_max) / 3))
    two = O.knn_mean_dist2(np.array([[0, 0, 0], [1, 0, 0]], np.float32))
    assert np.all(np.isinf(two))  # (1 + FLT_MAX + FLT_MAX) overflows in fp32, as upstream's sum


@pytest.mark.parametrize("P,W,H,deg,mod", [(2000, 96, 64, 3, 1.0), (3000, 130, 70, 1, 1.4)])
def test_torch_splat_baseline_matches_oracle(P, W, H, deg, mod):
    """The naive PyTorch-CPU splat (oracle/torch_splat.py, bench.py's cpu_baseline_torch leg) is
    an independent formulation -- upstream's exp(power), tensor ops, torch.autograd -- and must
    render and differentiate the same frame as the C oracle: radii bit-exact, PSNR >= 100 dB,
    gradients within 1e-4 relative L2."""
    _torch_splat_matches_oracle(O.synthetic_scene(P, W, H, seed=3, sh_degree=deg), P, W, H, deg, mod)


@pytest.mark.parametrize("P,W,H,deg,mod", [(2000, 96, 64, 3, 1.0), (3000, 130, 70, 1, 1.4)])
def test_torch_splat_baseline_matches_oracle_posed(P, W, H, deg, mod):
    """The same under the steep pose, with capped alphas and a wide SH DC term (posed_cases; no rows
    past the 1.3 * tanfov clamp: the splat's autograd differentiates through the clamped value, which
    upstream's backward holds fixed)."""
    import posed_cases as PC
    s = PC.populate(O.synthetic_scene(P, W, H, seed=3, sh_degree=deg), 3, opaque=0.2, dark=2.0)
    _torch_splat_matches_oracle(PC.pose_scene(s, PC.pose("steep", W, H)), P, W, H, deg, mod)


def _torch_splat_matches_oracle(s, P, W, H, deg, mod):
    import torch
    import torch_splat as TS
    rng = np.random.default_rng(1)
    dcol = (rng.normal(size=(3, H, W)) / (W * H)).astype(np.float32)
    dinv = (rng.normal(size=(1, H, W)) / (W * H)).astype(np.float32)
    st = O.forward(s["means3D"], s["opacities"], s["view"], s["proj"], s["campos"], s["bg"], W, H, s["tanfovx"],
                   s["tanfovy"], sh_degree=deg, shs=s["shs"], scales=s["scales"], rotations=s["rotations"],
                   scale_modifier=mod)
    og = O.backward(st, dcol, dinv)
    leaves, cam = TS.scene_tensors(s)
    color, invd, radii = TS.render(**leaves, **cam, scale_modifier=mod)
    ((color * torch.as_tensor(dcol)).sum() + (invd * torch.as_tensor(dinv)).sum()).backward()
    np.testing.assert_array_equal(radii.numpy(), st["radii"])
    mse = float(np.mean((color.detach().numpy() - st["color"]) ** 2))
    assert mse == 0 or 10 * np.log10(1.0 / mse) >= 100.0
    assert rel_l2(invd.detach().numpy(), st["invdepth"]) < 1e-5
    for k, ok in [("means3D", "dL_dmeans3D"), ("opacities", "dL_dopacity"), ("shs", "dL_dsh"),
                  ("rotations", "dL_drotations")]:
        assert rel_l2(leaves[k].grad.numpy().reshape(og[ok].shape), og[ok]) < 1e-4, k
    # upstream's dL/dscale omits the scale_modifier factor (oracle default): d/d(mod s) = grad / mod
    assert rel_l2(leaves["scales"].grad.numpy() / mod, og["dL_dscales"]) < 1e-4
