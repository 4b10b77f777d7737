"""GPU tests of the LOD hierarchy builder (csrc/hier_build.hip through gs_train.hier_build) against
its numpy restatement tests/hier_build_ref.py (the rule: DESIGN.md "Hierarchy builder"; parity
unpinned against the un-vendored gaussianhierarchy tool).

Exact: nodes, leaf_rows and levels equal the reference's; leaf rows are bit copies of the input; an
interior box is the bitwise union of the device's own children's boxes; boxes[:, 0, 3] is the fp32
largest extent of the device's own box.

Toleranced, and local so that error does not compound over the tree's ~40 levels: every interior
node's own two child rows, as the device wrote them, go through the float64 step E, and the device's
merged row is compared with that.  The bounds are 4 x the largest error a float32 numpy evaluation of
the same step shows against float64 on these same cases (hier_build_ref.fp32_basis(), run on a CPU;
`python tests/hier_build_ref.py` prints them) -- the margin covers another operation order, the
device's powf and its Jacobi iteration against eigh.  Nothing here is derived from the device's output.

The sizes: P = 64 / 65 straddle a wave, 1000 and 4097 several 256-node workgroups and 1024-node
numbering tiles.  P = 20 000 (39 999 nodes) crosses every single-workgroup and single-tile limit a
build of any size meets: the 256-node workgroups of the leaf and merge launches (157 of them, levels of
many workgroups), the 1024-node tiles of the numbering (levels of up to ~10 tiles, so the scanned tile
offsets are non-zero) and the 256-thread blocks of the bounds, key and topology launches.  Two loops
only run longer at sizes no test should reach -- the bounds launch's grid stride (past 524 288 rows) and
the tile-sum scan's rounds (past 1024 tiles: a level of a million nodes); both are the same code path
at any size.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hier_build_ref as R  # noqa: E402

DEV = "cuda"

# hier_build_ref.fp32_basis() over R.GPU_CASES, measured on a CPU (numpy float32 against float64):
# mu and SH relative to the larger child norm, opacity (W / S) relative, R diag(s^2) R^T against the
# mixture covariance in relative Frobenius norm, leaf box coordinates relative to the largest one.
FP32_MEASURED = dict(mu=1.701e-07, sh=1.969e-07, opacity=1.404e-04, cov=9.020e-07, leaf_box=6.777e-08)
BOUNDS = {k: 4.0 * v for k, v in FP32_MEASURED.items()}
UNIT_QUAT_TOL = 4 * 2.0 ** -23  # a normalised fp32 quaternion: a few roundings of the squared norm

_cache = {}


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _build(c, **kw):
    from gs_train.hier_build import build_hierarchy
    return build_hierarchy(_t(c["xyz"]), _t(c["log_scales"]), _t(c["rotations"]), _t(c["opacities"]), _t(c["shs"]), **kw)


def _np(h):
    return dict(means3D=h.means3D.cpu().numpy(), log_scales=h.log_scales.cpu().numpy(),
                rotations=h.rotations.cpu().numpy(), opacities=h.opacities.cpu().numpy(), shs=h.shs.cpu().numpy(),
                nodes=h.nodes.cpu().numpy(), boxes=h.boxes.cpu().numpy(), leaf_rows=h.leaf_rows.cpu().numpy(),
                levels=h.levels)


def _case(kind, P, M):
    """The cloud, the reference's topology and the device's hierarchy: built once, never modified."""
    if (kind, P, M) not in _cache:
        c = R.cloud(kind, P, M, seed=P)
        _cache[kind, P, M] = (c, R.topology(R.morton_keys(c["xyz"])), _np(_build(c)))
    return _cache[kind, P, M]


CASES = pytest.mark.parametrize("kind,P,M", R.GPU_CASES, ids=[f"{k}-{p}-M{m}" for k, p, m in R.GPU_CASES])


@pytest.mark.gpu
@CASES
def test_topology_and_layout_equal_the_reference(kind, P, M):
    c, (nodes, leaf_rows, levels), d = _case(kind, P, M)
    assert d["nodes"].shape == (2 * P - 1, 7) and d["nodes"].dtype == np.int32
    assert d["levels"] == levels
    assert np.array_equal(d["leaf_rows"], leaf_rows)
    assert np.array_equal(d["nodes"], nodes)


@pytest.mark.gpu
@CASES
def test_leaf_rows_are_bit_copies_and_boxes_are_exact_unions(kind, P, M):
    c, _, d = _case(kind, P, M)
    lr = d["leaf_rows"]
    leaf = lr >= 0
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for name, src in (("means3D", "xyz"), ("log_scales", "log_scales"), ("rotations", "rotations"),
                      ("opacities", "opacities"), ("shs", "shs")):
        assert np.array_equal(bits(d[name][leaf]), bits(c[src][lr[leaf]])), name
    b = d["boxes"]
    inner = np.nonzero(~leaf)[0]
    ca = d["nodes"][inner, 5]
    assert np.array_equal(bits(b[inner, 0, :3]), bits(np.minimum(b[ca, 0, :3], b[ca + 1, 0, :3])))
    assert np.array_equal(bits(b[inner, 1, :3]), bits(np.maximum(b[ca, 1, :3], b[ca + 1, 1, :3])))
    assert np.array_equal(bits(b[:, 0, 3]), bits(R.box_extent(b)))
    assert not b[:, 1, 3].any()


@pytest.mark.gpu
@CASES
def test_merged_rows_against_the_float64_step_on_the_devices_own_children(kind, P, M):
    c, _, d = _case(kind, P, M)
    lr = d["leaf_rows"]
    leaf = lr >= 0
    e_box = R.leaf_box_error(d["boxes"][leaf, 0, :3], d["boxes"][leaf, 1, :3], c["xyz"][lr[leaf]],
                             c["log_scales"][lr[leaf]], c["rotations"][lr[leaf]])
    idx, a, b, rows = R.children_of(d)
    got = {k: v[idx] for k, v in rows.items()}
    ref = R.merge_step(a, b)
    e = R.step_errors(got, ref, a, b)
    e["leaf_box"] = e_box
    print(kind, P, M, {k: f"{v:.3e}" for k, v in e.items()})
    for k, v in e.items():
        assert v <= BOUNDS[k], (k, v, BOUNDS[k])
    # W = 0 (both children transparent): weights 1/2 and opacity exactly 0
    dead = ~(np.isfinite(ref["W"]) & (ref["W"] > 0))
    assert not got["opacities"][dead].any()
    if kind == "zero_pair":
        assert dead.sum() > 0
    q = d["rotations"][~leaf].astype(np.float64)
    assert (np.abs((q * q).sum(1) - 1.0) <= UNIT_QUAT_TOL).all()
    assert np.isfinite(d["log_scales"]).all() and np.isfinite(d["means3D"]).all() and np.isfinite(d["opacities"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,P,M", [("random", 4097, 16), ("ties", 300, 16)])
def test_two_builds_are_bitwise_equal(kind, P, M):
    c, _, d = _case(kind, P, M)
    again = _np(_build(c))
    for k, v in d.items():
        if k == "levels":
            assert again[k] == v
        else:
            assert np.array_equal(np.ascontiguousarray(again[k]).view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), k


@pytest.mark.gpu
def test_first_row_leaves_the_skybox_out():
    c = R.cloud("random", 500, 4, seed=11)
    h = _np(_build(c, first_row=37))
    _, leaf_rows, levels = R.topology(R.morton_keys(c["xyz"][37:]))
    assert h["nodes"].shape[0] == 2 * 463 - 1 and h["levels"] == levels
    assert np.array_equal(h["leaf_rows"], np.where(leaf_rows >= 0, leaf_rows + 37, -1))
    leaf = h["leaf_rows"] >= 0
    assert np.array_equal(h["means3D"][leaf], c["xyz"][h["leaf_rows"][leaf]])


@pytest.mark.gpu
def test_non_finite_positions_are_refused():
    c = R.cloud("random", 50, 4, seed=2)
    c["xyz"][17, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        _build(c)


def _proper_cut(nodes, ni):
    N = nodes.shape[0]
    assert len(np.unique(ni)) == len(ni)
    cover = np.zeros(N, np.int64)
    cover[ni] = 1
    for n in range(1, N):  # parents are stored before their children
        cover[n] += cover[nodes[n, 1]]
    assert (cover[nodes[:, 6] == 0] == 1).all()


@pytest.fixture(scope="module")
def frustum():
    from gs_train.synthetic import camera
    c = R.cloud("random", 2000, 16, seed=21)
    return c, _build(c), camera(640, 360)


def _cut(h, target, campos):
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    N = h.nodes.shape[0]
    ri, pi, ni = (torch.zeros(N, dtype=torch.int32, device=DEV) for _ in range(3))
    w = torch.zeros(N, device=DEV)
    k = torch.zeros(N, dtype=torch.int32, device=DEV)
    cam = torch.tensor(campos, device=DEV)
    n = expand_to_size(h.nodes, h.boxes, target, cam, torch.zeros(3), ri, pi, ni)
    get_interpolation_weights(ni[:n], target, h.nodes, h.boxes, cam.cpu(), torch.zeros(3), w, k)
    return n, ri, pi, ni, w, k


@pytest.mark.gpu
def test_device_cut_of_a_built_hierarchy_is_proper_and_blends_exactly_at_target_zero(frustum):
    from gs_train.hier import interpolate_cut
    from gs_train.synthetic import tau_threshold
    c, h, (view, proj, campos, tx, ty) = frustum
    nodes = h.nodes.cpu().numpy()
    lengths = []
    for tau in (40.0, 10.0, 2.0):
        n, ri, pi, ni, w, k = _cut(h, float(np.float32(tau_threshold(tau, tx, 640))), campos)
        _proper_cut(nodes, ni[:n].cpu().numpy())
        assert torch.equal(ri[:n], ni[:n])
        lengths.append(n)
    assert 1 < lengths[0] < lengths[1] < lengths[2] <= 2000, lengths
    n, ri, pi, ni, w, k = _cut(h, 0.0, campos)
    assert n == 2000 and sorted(ni[:n].tolist()) == np.nonzero(nodes[:, 6] == 0)[0].tolist()
    assert bool(torch.all(w[:n] == 1.0)) and bool(torch.all(k[:n] == 2))
    cols = (h.means3D, torch.exp(h.log_scales), h.rotations, h.opacities, h.shs)
    out = interpolate_cut(*cols, ri[:n], pi, w, 0)
    for got, src in zip(out, cols):
        assert torch.equal(got, src[ri[:n].long()])  # t = 1: the leaf rows themselves, in cut order


@pytest.mark.gpu
def test_rasterizer_renders_a_cut_of_a_built_hierarchy(frustum):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gs_train.synthetic import tau_threshold
    c, h, (view, proj, campos, tx, ty) = frustum
    W, H = 640, 360
    n, ri, pi, ni, w, k = _cut(h, float(np.float32(tau_threshold(10.0, tx, W))), campos)
    assert 1 < n < 2000
    t = lambda x: torch.tensor(np.asarray(x), dtype=torch.float32, device=DEV)
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=float(tx), tanfovy=float(ty), bg=t([0.0, 0.0, 0.0]), scale_modifier=1.0,
        viewmatrix=t(view).reshape(4, 4), projmatrix=t(proj).reshape(4, 4), sh_degree=3, campos=t(campos),
        prefiltered=False, debug=False, do_depth=True, render_indices=ri[:n], parent_indices=pi,
        interpolation_weights=w, num_node_kids=k)
    N = h.means3D.shape[0]
    with torch.no_grad():
        color, radii, invd = GaussianRasterizer(rs)(
            means3D=h.means3D, means2D=torch.zeros(N, 3, device=DEV), shs=h.shs, opacities=h.opacities,
            scales=torch.exp(h.log_scales), rotations=torch.nn.functional.normalize(h.rotations))
    torch.cuda.synchronize()
    assert radii.shape[0] == n and int((radii > 0).sum()) > n // 2
    assert bool(torch.isfinite(color).all()) and bool(torch.isfinite(invd).all())
    assert float(color.abs().sum()) > 0 and float(invd.sum()) > 0


@pytest.mark.gpu
def test_post_train_step_on_a_built_hierarchy(frustum):
    from gs_train.post import PostTrainStep
    from gs_train.synthetic import orbit_cameras
    c, h, _ = frustum
    W, H = 320, 192
    sky = R.cloud("random", 30, 16, seed=5)
    sky["xyz"] *= 20.0
    model = h.to_model(tuple(_t(sky[k]) for k in ("xyz", "log_scales", "rotations", "opacities", "shs")))
    N = h.means3D.shape[0]
    assert model.N == N + 30 and model.skybox_points == 30
    assert torch.equal(model._xyz[:N], h.means3D) and torch.equal(model._xyz[N:], _t(sky["xyz"]))
    assert torch.equal(model._opacity[:N], h.opacities)
    g = torch.Generator(device=DEV).manual_seed(0)
    gts = [torch.rand(3, H, W, generator=g, device=DEV) for _ in range(2)]
    step = PostTrainStep(model, orbit_cameras(2, W, H), gts, W, H, iterations=100)
    step.limit_fn = lambda it: 0.02
    before = [p.detach().clone() for p in (model._xyz, model._features, model._opacity, model._scaling, model._rotation)]
    loss = step.step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and 0 < step.last_cut < N
    after = (model._xyz, model._features, model._opacity, model._scaling, model._rotation)
    for a_, b_ in zip(after, before):
        assert bool(torch.isfinite(a_).all()) and not torch.equal(a_[:N], b_[:N])
        assert torch.equal(a_[N:], b_[N:])  # the skybox rows are locked
    assert torch.equal(h.means3D, before[0][:N])  # the hierarchy's own tensors are not trained in place
