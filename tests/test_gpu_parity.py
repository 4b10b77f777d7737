"""GPU parity: the HIP path (through the public diff_gaussian_rasterization API) against the
CPU oracle (oracle/gs_oracle.c, itself checked against the reference's helpers and against
fp64 autograd in tests/test_oracle.py) on the same seeded inputs.

Bars (stated here, SURVEY.md 8 / BASELINE.json north_star):
  * integer / index work bit-exact: radii, tiles_touched, K, sorted 64-bit keys, point list,
    tile ranges;
  * n_contrib: exact except where an exp() ulp flips the alpha < 1/255 or T < 1e-4 test:
    mismatching pixel fraction <= NC_TOL;
  * colour / inverse depth: PSNR vs oracle >= PSNR_BAR, at most OFF_TOL of the pixels off by
    > 1e-4, inverse depth relative L2 <= INV_TOL;
  * gradients: relative L2 error <= GRAD_TOL per tensor (fp32, summation order differs).

The bars sit about 10x from what the kernels achieve (profiles/r04_parity_margins.jsonl, every
case of this file, test_gpu_metric.py and test_gpu_lod.py recorded on MI355X with
GSR_PARITY_RECORD): PSNR >= 157.8 dB, n_contrib mismatch <= 8.5e-7 (1-2 pixels of 2.4M), no pixel
off by 1e-4, inverse depth <= 2.4e-8 and gradients <= 4.9e-6 relative L2.  Round 2's quadratic
exponent (132 dB, 3.5e-4 gradient error) would fail them; only the drift test against upstream's
own exponent formulation (test_gpu_metric.py) keeps loose bars.
"""
from __future__ import annotations

import contextlib

import numpy as np
import pytest

from helpers import decode_state, psnr, record_margins, rel_l2, settings, torch_inputs

GRAD_TOL = 5e-5
PSNR_BAR = 145.0
NC_TOL = 1e-5
OFF_TOL = 1e-6
INV_TOL = 3e-7

CASES = [
    dict(name="tiny_deg3", P=300, W=64, H=48, deg=3, seed=1, log_scale=-2.5),
    dict(name="odd_size_deg1", P=800, W=70, H=50, deg=1, seed=2, log_scale=-2.8),
    dict(name="big_splats_deg0", P=200, W=96, H=64, deg=0, seed=3, log_scale=-1.3),
    dict(name="offcenter_modifier_deg2", P=2000, W=96, H=64, deg=2, seed=4, log_scale=-3.0, primx=0.4, primy=0.6,
         scale_modifier=1.7),
    dict(name="no_depth", P=1500, W=80, H=64, deg=3, seed=5, log_scale=-3.0, do_depth=False),
    dict(name="behind_camera", P=1500, W=96, H=64, deg=3, seed=6, log_scale=-3.0, behind=0.3),
    dict(name="coarse_M4", P=1500, W=96, H=64, deg=1, seed=7, log_scale=-3.0, M=4),
    dict(name="config1_10k_256", P=10000, W=256, H=256, deg=3, seed=0, log_scale=-4.0),
    # depth ties: 3000 Gaussians at one depth, ordered by id inside every tile
    dict(name="equal_depths", P=3000, W=96, H=64, deg=1, seed=9, log_scale=-3.0, flat_z=6.0),
    # many depth-sort tiles (8192 keys each) with ties across tiles and culled Gaussians mixed in
    dict(name="sort_tiles_ties", P=40000, W=128, H=96, deg=0, seed=14, log_scale=-3.5, behind=0.2, quant_z=0.25),
    # depth keys spanning more than 2^27 float steps (z 0.25 .. 1e5): the depth sort's 4 x 8-bit
    # layout (every other case fits the 3 x 9-bit one); culled Gaussians mixed in
    dict(name="wide_depth_4pass", P=4000, W=96, H=64, deg=1, seed=16, log_scale=-3.0, far=0.3, behind=0.1),
    # footprints over tens of 4x4-tile superblocks next to small ones (the binning's wave-wide path)
    dict(name="huge_splats_sb", P=300, W=640, H=480, deg=1, seed=15, log_scale=-0.5),
    # more than 255 tiles across: the 8-B tile rects (every other case packs them into 4 B)
    dict(name="wide_frame_rect8", P=3000, W=4200, H=64, deg=1, seed=17, log_scale=-3.0),
    # frame shapes at the grid's edges: one pixel, one partial tile, one-tile-wide column and
    # two-pixel-high row (superblock grids of 1 x n), a single Gaussian, and a 2 x 2 tile frame
    dict(name="single_pixel", P=60, W=1, H=1, deg=1, seed=18, log_scale=-2.0),
    dict(name="one_tile_15x17", P=200, W=15, H=17, deg=2, seed=19, log_scale=-2.5),
    dict(name="thin_column_3x300", P=400, W=3, H=300, deg=0, seed=20, log_scale=-2.5),
    dict(name="thin_row_500x2", P=400, W=500, H=2, deg=3, seed=21, log_scale=-2.5),
    dict(name="single_gaussian", P=1, W=48, H=40, deg=3, seed=22, log_scale=-1.0),
    dict(name="tile_edges_32x32", P=3000, W=32, H=32, deg=1, seed=23, log_scale=-3.2),
]


def make_scene(c):
    import gs_oracle as O
    s = O.synthetic_scene(c["P"], c["W"], c["H"], seed=c["seed"], sh_degree=3, log_scale_mean=c["log_scale"],
                          primx=c.get("primx", 0.5), primy=c.get("primy", 0.5), fovx_deg=c.get("fovx", 60.0))
    if c.get("M", 16) != 16:
        s["shs"] = np.ascontiguousarray(s["shs"][:, :c["M"], :])
    if c.get("flat_z"):
        m = s["means3D"]
        m[:, :2] *= c["flat_z"] / m[:, 2:3]  # same direction, one depth for every Gaussian
        m[:, 2] = c["flat_z"]
    if c.get("quant_z"):
        m = s["means3D"]
        z = np.maximum(np.round(m[:, 2] / c["quant_z"]), 1.0).astype(np.float32) * np.float32(c["quant_z"])
        m[:, :2] *= z[:, None] / m[:, 2:3]
        m[:, 2] = z
    if c.get("far"):
        # a fraction moved along its ray to z in [1e3, 1e5] (log-uniform), scaled to stay visible,
        # and one Gaussian pulled in to z = 0.25
        rng = np.random.default_rng(c["seed"] + 200)
        idx = np.nonzero(rng.random(c["P"]) < c["far"])[0]
        m = s["means3D"]
        znew = np.exp(rng.uniform(np.log(1e3), np.log(1e5), len(idx))).astype(np.float32)
        f = znew / m[idx, 2]
        m[idx] *= f[:, None]
        s["scales"][idx] *= f[:, None]
        f0 = np.float32(0.25) / m[0, 2]
        m[0] *= f0
        s["scales"][0] *= f0
    if c.get("behind"):
        rng = np.random.default_rng(c["seed"] + 100)
        idx = rng.random(c["P"]) < c["behind"]
        s["means3D"][idx, 2] = rng.uniform(-5.0, 0.25, idx.sum()).astype(np.float32)
    return s


def run_oracle(s, c, dcol, dinv, colors_precomp=None, cov3D_precomp=None):
    import gs_oracle as O
    st = O.forward(s["means3D"], s["opacities"], s["view"], s["proj"], s["campos"], s["bg"], s["W"], s["H"],
                   s["tanfovx"], s["tanfovy"], sh_degree=c["deg"],
                   shs=None if colors_precomp is not None else s["shs"], colors_precomp=colors_precomp,
                   scales=None if cov3D_precomp is not None else s["scales"],
                   rotations=None if cov3D_precomp is not None else s["rotations"], cov3D_precomp=cov3D_precomp,
                   scale_modifier=c.get("scale_modifier", 1.0), do_depth=c.get("do_depth", True))
    g = O.backward(st, dcol, dinv)
    return st, g


def run_hip(s, c, dcol, dinv, colors_precomp=None, cov3D_precomp=None):
    import torch
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    dev = torch.device("cuda:0")
    inp = torch_inputs(s, dev, use_precomp_colors=colors_precomp is not None,
                       use_precomp_cov=cov3D_precomp is not None, colors_precomp=colors_precomp,
                       cov3D_precomp=cov3D_precomp)
    rs = settings(s, dev, c["deg"], c.get("scale_modifier", 1.0), c.get("do_depth", True))
    # one raw _C call to get the scratch buffers for the bit-exact intermediate checks
    e = torch.empty(0, device=dev)
    raw = _C.rasterize_gaussians(rs.bg, inp["means3D"].detach(), inp.get("colors_precomp", e).detach(),
                                 inp["opacities"].detach(), inp.get("scales", e).detach(),
                                 inp.get("rotations", e).detach(), rs.scale_modifier,
                                 inp.get("cov3D_precomp", e).detach(), rs.viewmatrix, rs.projmatrix, rs.tanfovx,
                                 rs.tanfovy, rs.image_height, rs.image_width, inp.get("shs", e).detach(),
                                 rs.sh_degree, rs.campos, False, False, rs.render_indices, rs.parent_indices,
                                 rs.interpolation_weights, rs.num_node_kids, rs.do_depth)
    torch.cuda.synchronize()
    K = raw[0]
    state = decode_state(raw[4], raw[5], raw[6], c["P"], K, s["W"], s["H"])
    color, radii, invd = GaussianRasterizer(rs)(**inp)
    loss = (color * torch.tensor(dcol, device=dev)).sum()
    if c.get("do_depth", True):
        loss = loss + (invd * torch.tensor(dinv, device=dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (v.grad.detach().cpu().numpy() if v.grad is not None else None) for k, v in inp.items()}
    return dict(K=K, state=state, color=color.detach().cpu().numpy(), invdepth=invd.detach().cpu().numpy(),
                radii=radii.cpu().numpy(), grads=grads)


def check_record_offsets(S, vis, K):
    """The backward's Gaussian-major record bases (exclusive scan of tiles_touched in Gaussian
    order): the visible Gaussians' ranges [off, off + tiles_touched) partition [0, K) exactly."""
    off = S["offsets"][vis].astype(np.int64)
    n = S["tiles_touched"][vis].astype(np.int64)
    o = np.argsort(off, kind="stable")
    off, n = off[o], n[o]
    if len(off):
        assert off[0] == 0 and off[-1] + n[-1] == K
        np.testing.assert_array_equal(off[1:], off[:-1] + n[:-1])


def compare(c, st, g, h, check_grads=True, global_sort=False, subsets=None, bars=None):
    """subsets: {name: row mask} (posed_cases.subsets): every gradient tensor is also held to GRAD_TOL
    over the rows of each mask alone, and the SH clamp flags (one byte per row, bit ch set when
    channel ch clamped at zero: preprocess.hip) equal the oracle's on every row with radii > 0.
    bars: {margin name: bar} replacing this file's bar for that margin alone (psnr, nc_bad, frac_off,
    invdepth_rel_l2, grad_<input>, grad_<input>@<subset>): for cases on which the oracle itself
    stands further from fp64 than the bar (test_gpu_shapes.py states where its values come from)."""
    bar = lambda k, default: (bars or {}).get(k, default)
    assert h["K"] == st["K"], f"K {h['K']} vs oracle {st['K']}"
    np.testing.assert_array_equal(h["radii"], st["radii"])
    S = h["state"]
    if subsets is not None:
        on = st["radii"] > 0
        want = (st["clamped"].reshape(-1, 3).astype(np.uint8) << np.arange(3, dtype=np.uint8)).sum(1).astype(np.uint8)
        np.testing.assert_array_equal(S["clamped"][on], want[on])
    np.testing.assert_array_equal(S["tiles_touched"], st["tiles_touched"])
    np.testing.assert_array_equal(S["keys"], st["keys"])
    np.testing.assert_array_equal(S["point_list"], st["point_list"])
    np.testing.assert_array_equal(S["ranges"], st["ranges"])
    vis = (h["radii"] > 0) & (S["tiles_touched"] > 0)
    if global_sort:
        # the global depth order itself: visible Gaussians by (depth bits, id) (the culled ones are
        # not sorted: the slots past them are never read); and the Gaussian-major record offsets
        # its first pass writes
        nv = int(vis.sum())
        ids = np.nonzero(vis)[0]
        want = ids[np.lexsort((ids, S["depths"].view(np.uint32)[ids]))]
        np.testing.assert_array_equal(S["order"][:nv], want)
        check_record_offsets(S, vis, h["K"])
    # the raw (superblock-major) ranges partition [0, K) exactly
    r = S["ranges_raw"].astype(np.int64)
    o = np.argsort(r[:, 0], kind="stable")
    assert np.all(r[:, 1] >= r[:, 0])
    rs = r[o]
    nzr = rs[rs[:, 1] > rs[:, 0]]
    assert len(nzr) == 0 or (nzr[0, 0] == 0 and nzr[-1, 1] == h["K"] and np.all(nzr[1:, 0] == nzr[:-1, 1]))
    nc_bad = float(np.mean(S["n_contrib"] != st["n_contrib"]))
    p_img = psnr(h["color"], st["color"])
    off = float(np.mean(np.abs(h["color"] - st["color"]) > 1e-4))
    inv = rel_l2(h["invdepth"], st["invdepth"]) if c.get("do_depth", True) else None
    margins = dict(psnr=p_img if np.isfinite(p_img) else 999.0, nc_bad=nc_bad, frac_off=off, invdepth_rel_l2=inv)
    try:
        assert nc_bad <= bar("nc_bad", NC_TOL), f"n_contrib mismatch fraction {nc_bad}"
        assert p_img >= bar("psnr", PSNR_BAR), p_img
        assert off <= bar("frac_off", OFF_TOL), off
        if inv is not None:
            assert inv <= bar("invdepth_rel_l2", INV_TOL), inv
        if not check_grads:
            return
        G = h["grads"]
        pairs = [("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity")]
        if G.get("shs") is not None:
            pairs.append(("shs", "dL_dsh"))
        if G.get("colors_precomp") is not None:
            pairs.append(("colors_precomp", "dL_dcolors"))
        if G.get("scales") is not None:
            pairs += [("scales", "dL_dscales"), ("rotations", "dL_drotations")]
        if G.get("cov3D_precomp") is not None:
            pairs.append(("cov3D_precomp", "dL_dcov3D"))
        for hk, ok in pairs:
            err = rel_l2(G[hk].reshape(g[ok].shape), g[ok])
            margins["grad_" + hk] = err
            assert err <= bar("grad_" + hk, GRAD_TOL), f"{c['name']}: grad {hk} rel L2 {err}"
            for name, m in (subsets or {}).items():
                err = rel_l2(G[hk].reshape(g[ok].shape)[m], g[ok][m])
                margins[f"grad_{hk}@{name}"] = err
                assert err <= bar(f"grad_{hk}@{name}", GRAD_TOL), \
                    f"{c['name']}: grad {hk} over the {int(m.sum())} {name} rows rel L2 {err}"
    finally:
        record_margins(c["name"], **margins)
    return


def upstream_grads(c, seed=99):
    rng = np.random.default_rng(seed)
    n = c["W"] * c["H"]
    return ((rng.normal(size=(3, c["H"], c["W"])) / n * 1e3).astype(np.float32),
            (rng.normal(size=(1, c["H"], c["W"])) / n * 1e3).astype(np.float32))


@contextlib.contextmanager
def binning_mode(mode):
    """gsr_set_binning for the duration: 0 = local per-superblock sort, 1 = global sort (default)."""
    from diff_gaussian_rasterization import _C
    prev = _C.set_binning(mode)
    try:
        yield
    finally:
        _C.set_binning(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["local_sort", "global_sort"])
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_parity_vs_oracle(c, mode):
    s = make_scene(c)
    dcol, dinv = upstream_grads(c)
    st, g = run_oracle(s, c, dcol, dinv)
    with binning_mode(mode):
        h = run_hip(s, c, dcol, dinv)
    compare(c, st, g, h, global_sort=mode == 1)


@pytest.mark.gpu
def test_local_sort_paths_and_fallback():
    """The binning's two depth-order strategies give identical frames: a sparse frame is binned by
    the local (per-superblock LDS) sort, a frame with a superblock list longer than the LDS sort
    holds falls back to the global sort (gsr_forward_stats counts both), and both equal the forced
    global sort bit for bit (image, inverse depth, radii, tile lists)."""
    import torch
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    dev = torch.device("cuda:0")
    for c, expect_fallback in ((dict(name="sparse", P=20000, W=320, H=240, deg=3, seed=41, log_scale=-3.5), False),
                               (dict(name="dense_sb", P=60000, W=160, H=96, deg=1, seed=42, log_scale=-3.5), True)):
        s = make_scene(c)
        outs = []
        for mode in (0, 1):
            with binning_mode(mode), torch.no_grad():
                inp = torch_inputs(s, dev, requires_grad=False)
                rs = settings(s, dev, c["deg"])
                f0 = _C.forward_stats()
                color, radii, invd = GaussianRasterizer(rs)(**inp)
                e = torch.empty(0, device=dev)
                raw = _C.rasterize_gaussians(rs.bg, inp["means3D"], e, inp["opacities"], inp["scales"],
                                             inp["rotations"], 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx,
                                             rs.tanfovy, rs.image_height, rs.image_width, inp["shs"], c["deg"],
                                             rs.campos, False, False, rs.render_indices, rs.parent_indices,
                                             rs.interpolation_weights, rs.num_node_kids, True)
                torch.cuda.synchronize()
                f1 = _C.forward_stats()
                st = decode_state(raw[4], raw[5], raw[6], c["P"], raw[0], s["W"], s["H"])
                outs.append((color.cpu(), invd.cpu(), radii.cpu(), st["point_list"], st["ranges"]))
                if mode == 0:
                    assert f1["local_sort"] - f0["local_sort"] == (0 if expect_fallback else 2), (c["name"], f0, f1)
                    assert f1["fallbacks"] - f0["fallbacks"] == (2 if expect_fallback else 0), (c["name"], f0, f1)
                else:
                    assert f1["local_sort"] == f0["local_sort"] and f1["fallbacks"] == f0["fallbacks"]
        (a, b) = outs
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        np.testing.assert_array_equal(a[3], b[3])
        np.testing.assert_array_equal(a[4], b[4])


def precomputed_inputs(s, deg):
    """The reference's python paths in fp64: (colors_precomp from eval_sh + 0.5 clamped at zero,
    cov3D_precomp from get_covariance), as float32 arrays."""
    import dense_torch as DT
    import torch
    means = torch.tensor(s["means3D"], dtype=torch.float64)
    d = means - torch.tensor(s["campos"], dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    colors = torch.clamp_min(DT.eval_sh_t(deg, torch.tensor(s["shs"], dtype=torch.float64), d) + 0.5, 0.0)
    colors = colors.float().numpy()
    L = DT.quat_to_R(torch.tensor(s["rotations"], dtype=torch.float64)) * torch.tensor(
        s["scales"], dtype=torch.float64)[:, None, :]
    S3 = (L @ L.transpose(1, 2)).numpy()
    cov = np.stack([S3[:, 0, 0], S3[:, 0, 1], S3[:, 0, 2], S3[:, 1, 1], S3[:, 1, 2], S3[:, 2, 2]], 1)
    return colors, cov.astype(np.float32)


@pytest.mark.gpu
def test_precomputed_paths_and_cross_identity():
    """colors_precomp / cov3D_precomp paths against the oracle, and the cross-path identity
    pinned by reference code: rasterizing (shs, scales, rotations) equals rasterizing the
    reference's python paths (eval_sh + 0.5 clamp, get_covariance) -- SURVEY.md 8(c)(ii)."""
    c = dict(name="precomp", P=1500, W=96, H=64, deg=3, seed=11, log_scale=-3.0)
    s = make_scene(c)
    dcol, dinv = upstream_grads(c)
    colors, cov = precomputed_inputs(s, 3)
    st, g = run_oracle(s, c, dcol, dinv, colors_precomp=colors, cov3D_precomp=cov)
    h = run_hip(s, c, dcol, dinv, colors_precomp=colors, cov3D_precomp=cov)
    compare(c, st, g, h)
    base = run_hip(s, c, dcol, dinv)
    assert psnr(base["color"], h["color"]) > 60.0
    assert float(np.mean(base["radii"] != h["radii"])) < 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize("deterministic", [True, False])
def test_boundary_contract_and_determinism(deterministic):
    """Output contract; with gsr_set_deterministic(1) fwd+bwd is bitwise reproducible (records summed
    in a fixed order), in the default atomic mode the forward is and the gradients agree to fp32
    rounding of the summation order."""
    import torch
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    c = dict(name="contract", P=3000, W=120, H=72, deg=3, seed=12, log_scale=-3.2)
    s = make_scene(c)
    dev = torch.device("cuda:0")
    outs = []
    prev = _C.set_deterministic(deterministic)
    try:
        _contract_runs(s, dev, outs)
    finally:
        _C.set_deterministic(prev)
    for n, (a, b) in enumerate(zip(*outs)):
        if deterministic or n == 0:  # n == 0: the image
            assert torch.equal(a, b), "fwd+bwd must be bitwise reproducible in deterministic mode"
        else:
            assert float((a - b).norm() / max(float(b.norm()), 1e-30)) < 1e-5


def _contract_runs(s, dev, outs):
    import torch
    from diff_gaussian_rasterization import GaussianRasterizer
    for _ in range(2):
        inp = torch_inputs(s, dev)
        inp["means2D"].retain_grad()
        rs = settings(s, dev, 3)
        color, radii, invd = GaussianRasterizer(rs)(**inp)
        assert color.shape == (3, 72, 120) and color.dtype == torch.float32
        assert radii.shape == (3000,) and radii.dtype == torch.int32
        assert invd.shape == (1, 72, 120) and invd.dtype == torch.float32
        (color.sum() + invd.sum()).backward()
        g2 = inp["means2D"].grad
        assert torch.all(g2[:, 2] == 0)
        vis = radii > 0
        assert torch.all(g2[~vis] == 0)
        outs.append([color.detach().cpu()] + [v.grad.detach().cpu() for v in inp.values()])


@pytest.mark.gpu
def test_empty_and_degenerate_inputs():
    import torch
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    dev = torch.device("cuda:0")
    c = dict(name="empty", P=0, W=40, H=30, deg=0, seed=0, log_scale=-3.0)
    s = make_scene(dict(c, P=10))
    rs = settings(s, dev, 0)
    inp = dict(means3D=torch.zeros(0, 3, device=dev, requires_grad=True),
               means2D=torch.zeros(0, 3, device=dev, requires_grad=True),
               opacities=torch.zeros(0, 1, device=dev, requires_grad=True),
               shs=torch.zeros(0, 16, 3, device=dev, requires_grad=True),
               scales=torch.zeros(0, 3, device=dev, requires_grad=True),
               rotations=torch.zeros(0, 4, device=dev, requires_grad=True))
    color, radii, invd = GaussianRasterizer(rs)(**inp)
    bg = torch.tensor(s["bg"], device=dev)
    assert torch.allclose(color, bg[:, None, None].expand(3, 30, 40))
    assert radii.numel() == 0
    color.sum().backward()
    # all Gaussians behind the camera: K == 0 but the image is background
    s2 = make_scene(dict(name="behind", P=50, W=40, H=30, deg=0, seed=1, log_scale=-3.0))
    s2["means3D"][:, 2] = -3.0
    inp2 = torch_inputs(s2, dev)
    color2, radii2, _ = GaussianRasterizer(settings(s2, dev, 0))(**inp2)
    assert int((radii2 > 0).sum()) == 0
    assert torch.allclose(color2, torch.tensor(s2["bg"], device=dev)[:, None, None].expand(3, 30, 40))
    color2.sum().backward()
    assert torch.all(inp2["means3D"].grad == 0)
    vis = _C.mark_visible(inp2["means3D"].detach(), settings(s2, dev, 0).viewmatrix, settings(s2, dev, 0).projmatrix)
    assert not bool(vis.any())


@pytest.mark.gpu
def test_input_validation_errors():
    import torch
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    s = make_scene(dict(name="v", P=20, W=32, H=32, deg=0, seed=0, log_scale=-3.0))
    inp = torch_inputs(s, dev, requires_grad=False)
    rs = settings(s, dev, 0)
    with pytest.raises(Exception, match="one of either SHs or precomputed colors"):
        GaussianRasterizer(rs)(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                               scales=inp["scales"], rotations=inp["rotations"])
    with pytest.raises(Exception, match="scale/rotation pair"):
        GaussianRasterizer(rs)(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                               shs=inp["shs"], scales=inp["scales"])
    with pytest.raises(RuntimeError, match="means3D must have dimensions"):
        GaussianRasterizer(rs)(means3D=inp["means3D"][:, :2], means2D=inp["means2D"], opacities=inp["opacities"],
                               shs=inp["shs"], scales=inp["scales"], rotations=inp["rotations"])


@pytest.mark.gpu
def test_config2_full_size_vs_oracle():
    """Config 2 (500k Gaussians, 1920x1080): full-size bit-exact binning + image/gradient parity,
    plus size-independent structure checks (sortedness, range partition)."""
    c = dict(name="config2", P=500_000, W=1920, H=1080, deg=3, seed=0, log_scale=-4.0)
    s = make_scene(c)
    dcol, dinv = upstream_grads(c)
    st, g = run_oracle(s, c, dcol, dinv)
    h = run_hip(s, c, dcol, dinv)
    S = h["state"]
    keys = S["keys"]
    assert np.all(keys[1:] >= keys[:-1])
    r = S["ranges"]
    nz = r[:, 1] > r[:, 0]
    assert int((r[nz, 1] - r[nz, 0]).sum()) == h["K"]
    compare(c, st, g, h)


@pytest.mark.gpu
@pytest.mark.parametrize("deg,seed", [(3, 3), (1, 4)])
def test_street_frame_1536_vs_oracle(deg, seed):
    """The Street-sparse training frame: a 1536x1536 cube face with a 90 deg field of view
    (ss_utils/generate_colmap_calibration.py:306-308,476-479,572 -- SIMPLE_PINHOLE, f = size / 2 --
    below the 1600-px rescale of utils/camera_utils.py:64-81): 96 x 96 tiles, 576 superblocks,
    1M Gaussians.  Bit-exact binning (keys, point list, ranges), image PSNR and gradients vs the
    oracle; SH degree 1 is the coarse model's (train_coarse.py:31)."""
    c = dict(name=f"street1536_deg{deg}", P=1_000_000, W=1536, H=1536, deg=deg, seed=seed, log_scale=-4.0,
             fovx=90.0)
    s = make_scene(c)
    dcol, dinv = upstream_grads(c)
    st, g = run_oracle(s, c, dcol, dinv)
    h = run_hip(s, c, dcol, dinv)
    assert h["K"] > 2_000_000
    compare(c, st, g, h)


@pytest.mark.gpu
def test_street_frame_3M_culled_vs_oracle():
    """A street-chunk-sized frame: 3M Gaussians on a 1536x1536 90-degree view, 70% of them behind
    the camera (a cube face of a late street chunk culls about that share): the depth sort and the
    level-1 binning skip the culled rows (dsort.hip, binning.hip), and the sort fills the chip, so
    the SH colour pass forks after it.  Bit-exact binning, image and gradients vs the oracle."""
    c = dict(name="street1536_3M_culled", P=3_000_000, W=1536, H=1536, deg=3, seed=8, log_scale=-4.5, fovx=90.0,
             behind=0.7)
    s = make_scene(c)
    dcol, dinv = upstream_grads(c)
    st, g = run_oracle(s, c, dcol, dinv)
    h = run_hip(s, c, dcol, dinv)
    assert int((h["radii"] > 0).sum()) < 0.4 * c["P"]
    compare(c, st, g, h, global_sort=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n_vis", [0, 1, 8191, 8192, 8193, 16385])
def test_sort_tile_boundaries_with_culled_rows(n_vis):
    """Visible-row counts at the depth sort's 8192-key tile boundaries: the culled rows (key
    0xFFFFFFFF) are counted by the upsweep and left out of the passes, which run ceil(visible / 8192)
    tiles (dsort.hip), and the level-1 binning stops at the last visible chunk (binning.hip).  20000
    rows, the first n_vis on screen and the rest behind the camera, through the global sort;
    bit-exact binning and order, image and gradients vs the oracle."""
    c = dict(name=f"sort_tile_edge_{n_vis}", P=20000, W=128, H=96, deg=1, seed=30, log_scale=-3.5)
    s = make_scene(c)
    rng = np.random.default_rng(31)
    m = s["means3D"]
    z = rng.uniform(2.0, 10.0, c["P"]).astype(np.float32)
    m[:, 0] = z * rng.uniform(-0.6, 0.6, c["P"]).astype(np.float32) * np.float32(s["tanfovx"])
    m[:, 1] = z * rng.uniform(-0.6, 0.6, c["P"]).astype(np.float32) * np.float32(s["tanfovy"])
    m[:, 2] = z
    m[n_vis:, 2] = -z[n_vis:]  # behind the camera: culled
    dcol, dinv = upstream_grads(c)
    st, g = run_oracle(s, c, dcol, dinv)
    with binning_mode(1):
        h = run_hip(s, c, dcol, dinv)
    assert int(((h["radii"] > 0) & (h["state"]["tiles_touched"] > 0)).sum()) == n_vis
    compare(c, st, g, h, global_sort=True)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [10_000, 600_000])
def test_live_list_walk_same_bits(P):
    """gsr_set_live_list: the backward's live rows walked through one list spread over the chip give
    the bits the per-range walk gives (deterministic mode: record sums in a fixed order), here with
    more live rows than the list grid's threads (600k tiny splats at 1080p: several trips each), and
    the list's counters come back to zero for the next frame."""
    import torch
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    c = dict(name=f"live_list_{P}", P=P, W=1920 if P > 100_000 else 256, H=1080 if P > 100_000 else 256, deg=3,
             seed=40, log_scale=-4.6 if P > 100_000 else -4.0)
    s = make_scene(c)
    dev = torch.device("cuda:0")
    dcol, dinv = upstream_grads(c)
    prev = _C.set_deterministic(True)
    prev_ll = _C.set_live_list(False)
    try:
        out = {}
        for mode in (False, True, True, False):
            _C.set_live_list(mode)
            inp = torch_inputs(s, dev)
            color, radii, invd = GaussianRasterizer(settings(s, dev, 3))(**inp)
            loss = (color * torch.tensor(dcol, device=dev)).sum() + (invd * torch.tensor(dinv, device=dev)).sum()
            loss.backward()
            out.setdefault(mode, []).append({k: v.grad.clone() for k, v in inp.items()})
    finally:
        _C.set_deterministic(prev)
        _C.set_live_list(prev_ll)
    ref = out[False][0]
    for run in out[False][1:] + out[True]:
        for k in ref:
            assert torch.equal(ref[k], run[k]), k
    live = int((ref["opacities"] != 0).sum())  # nonzero for every live row
    assert live > (2 * 256 * 256 if P > 100_000 else 1000), live


@pytest.mark.gpu
def test_depth_order_large():
    """The global depth sort at 3M Gaussians (367 sort tiles) with 25% culled: the order's first
    slots are the stable (depth bits, id) order of the visible Gaussians (the culled ones are not
    sorted: nothing reads the slots past them); the record offsets partition [0, K); K is the sum
    of tiles_touched."""
    import torch
    from diff_gaussian_rasterization import _C
    c = dict(name="large", P=3_000_000, W=1920, H=1080, deg=0, seed=21, log_scale=-4.0, behind=0.25)
    s = make_scene(c)
    dev = torch.device("cuda:0")
    inp = torch_inputs(s, dev)
    rs = settings(s, dev, 0)
    e = torch.empty(0, device=dev)
    with torch.no_grad(), binning_mode(1):  # the global depth sort's own outputs (order, offsets)
        raw = _C.rasterize_gaussians(rs.bg, inp["means3D"], e, inp["opacities"], inp["scales"], inp["rotations"], 1.0,
                                     e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height,
                                     rs.image_width, inp["shs"], 0, rs.campos, False, False, rs.render_indices,
                                     rs.parent_indices, rs.interpolation_weights, rs.num_node_kids, True)
    torch.cuda.synchronize()
    K = int(raw[0])
    g = raw[4].cpu().numpy()
    from helpers import geom_layout, view
    gl = geom_layout(c["P"])
    rec = view(g, gl, "rec", np.float32, (c["P"], 16))
    tiles = view(g, gl, "tiles", np.uint32)
    order = view(g, gl, "order", np.uint32)
    offsets = view(g, gl, "offsets", np.uint32)
    radii = raw[3].cpu().numpy()
    vis = (radii > 0) & (tiles > 0)
    nv = int(vis.sum())
    assert 0 < nv < c["P"]
    assert K == int(tiles.astype(np.int64).sum())
    ids = np.nonzero(vis)[0]
    dbits = rec[:, 14].view(np.uint32)
    np.testing.assert_array_equal(order[:nv], ids[np.lexsort((ids, dbits[ids]))])
    check_record_offsets(dict(offsets=offsets, tiles_touched=tiles), vis, K)


@pytest.mark.gpu
def test_scratch_is_released_every_frame():
    """Scratch buffers must go back to the caching allocator when autograd releases them (no
    reference cycles through the ctypes resize callbacks)."""
    import torch
    from diff_gaussian_rasterization import GaussianRasterizer
    c = dict(name="mem", P=20000, W=320, H=240, deg=3, seed=13, log_scale=-3.5)
    s = make_scene(c)
    dev = torch.device("cuda:0")
    inp = torch_inputs(s, dev)
    rs = settings(s, dev, 3)

    def step():
        for v in inp.values():
            v.grad = None
        color, radii, invd = GaussianRasterizer(rs)(**inp)
        (color.sum() + invd.sum()).backward()

    step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(dev) <= base + (1 << 20)


@pytest.mark.gpu
@pytest.mark.parametrize("live_list", [False, True], ids=["per_range", "live_list"])
@pytest.mark.parametrize("deterministic", [False, True])
def test_backward_twice_through_saved_buffers(deterministic, live_list):
    """A second backward through the same forward (loss.backward(retain_graph=True) twice,
    torch.autograd.grad twice, gradcheck-style reuse) returns the same gradients: upstream's
    backward keeps no state between calls, render_bwd's accumulator rows are cleared by the
    pass that consumes them, and the live-row list's counters (gsr_set_live_list) by the last
    workgroup that walks it."""
    import torch
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    c = dict(name="twice", P=4000, W=128, H=96, deg=3, seed=31, log_scale=-3.2)
    s = make_scene(c)
    dev = torch.device("cuda:0")
    dcol, dinv = upstream_grads(c)
    prev = _C.set_deterministic(deterministic)
    prev_ll = _C.set_live_list(live_list)
    try:
        inp = torch_inputs(s, dev)
        color, radii, invd = GaussianRasterizer(settings(s, dev, 3))(**inp)
        loss = (color * torch.tensor(dcol, device=dev)).sum() + (invd * torch.tensor(dinv, device=dev)).sum()
        leaves = list(inp.values())
        g1 = torch.autograd.grad(loss, leaves, retain_graph=True)
        g2 = torch.autograd.grad(loss, leaves, retain_graph=True)
        loss.backward(retain_graph=True)
        g3 = [v.grad.clone() for v in leaves]
    finally:
        _C.set_deterministic(prev)
        _C.set_live_list(prev_ll)
    for a, b, d in zip(g1, g2, g3):
        if deterministic:
            assert torch.equal(a, b) and torch.equal(a, d)
        else:
            for x in (b, d):
                assert float((a - x).norm() / max(float(a.norm()), 1e-30)) < 1e-5
    assert float(g1[0].norm()) > 0


@pytest.mark.gpu
def test_no_grad_forward_skips_backward_state():
    """A frame autograd does not record (torch.no_grad) renders the same image, and its buffers
    are refused by the backward (GSR_FWD_NO_BACKWARD: accumulators not cleared)."""
    import torch
    from diff_gaussian_rasterization import GaussianRasterizer, _C
    c = dict(name="nograd", P=3000, W=96, H=64, deg=3, seed=32, log_scale=-3.0)
    s = make_scene(c)
    dev = torch.device("cuda:0")
    inp = torch_inputs(s, dev)
    rs = settings(s, dev, 3)
    color, radii, invd = GaussianRasterizer(rs)(**inp)
    with torch.no_grad():
        color2, radii2, invd2 = GaussianRasterizer(rs)(**inp)
    assert torch.equal(color, color2) and torch.equal(radii, radii2) and torch.equal(invd, invd2)
    e = torch.empty(0, device=dev)
    d = {k: v.detach() for k, v in inp.items()}
    raw = _C.rasterize_gaussians(rs.bg, d["means3D"], e, d["opacities"], d["scales"], d["rotations"], 1.0, e,
                                 rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width,
                                 d["shs"], 3, rs.campos, False, False, rs.render_indices, rs.parent_indices,
                                 rs.interpolation_weights, rs.num_node_kids, True, need_backward=False)
    assert torch.equal(raw[1], color2)
    with pytest.raises(RuntimeError, match="GSR_FWD_NO_BACKWARD"):
        _C.rasterize_gaussians_backward(rs.bg, d["means3D"], raw[3], e, d["scales"], d["rotations"], 1.0, e,
                                        rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy,
                                        torch.ones_like(raw[1]), None, d["shs"], 3, rs.campos, raw[4], raw[0], raw[5],
                                        raw[6], rs.render_indices, rs.parent_indices, rs.interpolation_weights,
                                        rs.num_node_kids, False)
