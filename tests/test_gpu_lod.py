"""GPU parity of the hierarchy LOD cut (csrc/lod.hip through the gaussian_hierarchy drop-in) with its
C restatement (oracle/gs_oracle.c; parity unpinned against the un-vendored gaussianhierarchy
extension -- see tests/test_lod_cpu.py for what pins the restatement), and config 5 end to end:
render_hierarchy.py's per-frame work -- expand_to_size at a tau threshold, get_interpolation_weights,
render_post's blend, the forward render at 1080p -- on a synthetic 10M-node hierarchy, against the
oracle on the same rows (bit-exact cut, weights, radii, K and tile lists; PSNR >= 137 dB)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import hier_ref
from helpers import psnr, record_margins

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _cut_hip(h, thr, vp=None):
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    N = h["nodes"].shape[0]
    ri, pi, ni = (torch.zeros(N, dtype=torch.int32, device=DEV) for _ in range(3))
    w = torch.zeros(N, device=DEV)
    k = torch.zeros(N, dtype=torch.int32, device=DEV)
    cam = torch.tensor(h["campos"] if vp is None else vp, device=DEV)
    n = expand_to_size(h["nodes"], h["boxes"], thr, cam, torch.zeros(3), ri, pi, ni)
    get_interpolation_weights(ni[:n], thr, h["nodes"], h["boxes"], cam.cpu(), torch.zeros(3), w, k)
    return n, ri, pi, ni, w, k


@pytest.mark.parametrize("tau,vp", [(3.0, None), (15.0, None), (60.0, (0.3, 0.1, 4.0)), (6.0, (0.0, 0.0, -50.0))])
def test_lod_cut_matches_oracle(tau, vp):
    import gs_oracle as O
    from gs_train.synthetic import synthetic_lod_hierarchy, tau_threshold
    h = synthetic_lod_hierarchy(400_000, 1920, 1080, DEV, seed=7, zmin=1.0, zmax=30.0, log_scale_mean=-3.5)
    thr = float(np.float32(tau_threshold(tau, h["tanfovx"], 1920)))
    n, ri, pi, ni, w, k = _cut_hip(h, thr, vp)
    nodes, boxes = h["nodes"].cpu().numpy(), h["boxes"].cpu().numpy()
    v = np.asarray(h["campos"] if vp is None else vp, np.float32)
    ori, opi, oni = O.expand_to_size(nodes, boxes, np.float32(thr), v)
    ow, ok = O.interpolation_weights(oni, np.float32(thr), nodes, boxes, v)
    assert n == len(ori) and n > 0
    np.testing.assert_array_equal(ri[:n].cpu().numpy(), ori)
    np.testing.assert_array_equal(pi[:n].cpu().numpy(), opi)
    np.testing.assert_array_equal(ni[:n].cpu().numpy(), oni)
    np.testing.assert_array_equal(w[:n].cpu().numpy(), ow)
    np.testing.assert_array_equal(k[:n].cpu().numpy(), ok)
    # outputs beyond the cut are untouched (the reference slices [:to_render])
    assert int(ri[n:].abs().sum()) == 0 and float(w[n:].abs().sum()) == 0.0


@pytest.mark.parametrize("leaves,offset", [(600, 0), (5000, 1), (70_000, 3)])
def test_lod_cut_ragged_tiles_and_unaligned_nodes(leaves, offset):
    """The cut (lod.hip: lod_cut_count_kernel's per-tile counts, records and sums over 1024-node tiles,
    lod_cut_write_kernel's offsets from the group and tile sums) on one ragged tile, on several, and
    with the nodes array starting `offset` rows into its buffer (28-B rows: not 16-B aligned) --
    bit-exact with the oracle."""
    import gs_oracle as O
    from gs_train.synthetic import synthetic_lod_hierarchy, tau_threshold
    h = synthetic_lod_hierarchy(leaves, 640, 360, DEV, seed=13, zmin=1.0, zmax=20.0, log_scale_mean=-3.0)
    N = h["nodes"].shape[0]
    if offset:
        buf = torch.zeros(N + offset, 7, dtype=torch.int32, device=DEV)
        buf[offset:] = h["nodes"]
        h = dict(h, nodes=buf[offset:])
        assert h["nodes"].data_ptr() % 16 != 0
    thr = float(np.float32(tau_threshold(10.0, h["tanfovx"], 640)))
    n, ri, pi, ni, w, k = _cut_hip(h, thr)
    nodes, boxes = h["nodes"].cpu().numpy(), h["boxes"].cpu().numpy()
    ori, opi, oni = O.expand_to_size(nodes, boxes, np.float32(thr), np.asarray(h["campos"], np.float32))
    assert n == len(ori) and 0 < n < N
    np.testing.assert_array_equal(ri[:n].cpu().numpy(), ori)
    np.testing.assert_array_equal(pi[:n].cpu().numpy(), opi)
    np.testing.assert_array_equal(ni[:n].cpu().numpy(), oni)
    assert int(ri[n:].abs().sum()) == 0


@pytest.mark.parametrize("case", ["root_small", "root_big", "empty", "multi_tile_empty_tiles"])
def test_lod_cut_edge_cases(case):
    """The two-launch cut on degenerate hierarchies, against the oracle: a lone root that fits the
    target (it renders its leaf and merged Gaussians), a lone root that is too big (its leaves
    only), a cut with nothing to render (every node too big, no leaf Gaussians), and 3000 nodes whose
    first tiles render nothing (whole tiles of zero counts before and after the rendered ones)."""
    import gs_oracle as O
    from gaussian_hierarchy._C import expand_to_size
    cam = np.zeros(3, np.float32)
    if case in ("root_small", "root_big", "empty"):
        nodes = np.array([[0, -1, 5, 2 if case != "empty" else 0, 3, -1, 0]], np.int32)
        boxes = np.zeros((1, 2, 4), np.float32)
        if case == "root_small":  # a small box far away: size / distance below the target
            boxes[0, 0, :3], boxes[0, 0, 3], boxes[0, 1, :3] = 99.0, 0.01, 100.0
        else:  # the viewpoint inside the box: +inf size, always too big
            boxes[0, 0, :3], boxes[0, 0, 3], boxes[0, 1, :3] = -1.0, 2.0, 1.0
    else:
        N = 3000
        nodes = np.zeros((N, 7), np.int32)
        nodes[:, 1] = -1
        nodes[:, 2] = np.arange(N)
        nodes[:, 4] = 1  # merged Gaussian each; rendered only when small
        boxes = np.zeros((N, 2, 4), np.float32)
        boxes[:, 0, :3], boxes[:, 0, 3], boxes[:, 1, :3] = -1.0, 2.0, 1.0  # contains the viewpoint
        small = np.arange(N)[(np.arange(N) >= 1500) & (np.arange(N) < 2100)]  # tiles 1-2 only
        boxes[small, 0, :3], boxes[small, 0, 3], boxes[small, 1, :3] = 99.0, 0.01, 100.0
    N = nodes.shape[0]
    thr = np.float32(0.5)
    dn, db = torch.tensor(nodes, device=DEV), torch.tensor(boxes, device=DEV)
    ri, pi, ni = (torch.full((N + 8,), -7, dtype=torch.int32, device=DEV) for _ in range(3))
    n = expand_to_size(dn, db, float(thr), torch.tensor(cam, device=DEV), torch.zeros(3), ri, pi, ni)
    ori, opi, oni = O.expand_to_size(nodes, boxes, thr, cam)
    assert n == len(ori), (n, len(ori))
    assert n == {"root_small": 5, "root_big": 2, "empty": 0, "multi_tile_empty_tiles": 600}[case]
    np.testing.assert_array_equal(ri[:n].cpu().numpy(), ori)
    np.testing.assert_array_equal(pi[:n].cpu().numpy(), opi)
    np.testing.assert_array_equal(ni[:n].cpu().numpy(), oni)
    assert bool(torch.all(ri[n:] == -7))


def _covered_once(h, ri, n):
    """Every leaf of the tree is rendered exactly once: by itself or through exactly one ancestor
    in the cut (each node holds one Gaussian, Gaussian i = node i).  Level by level on the device:
    cover[i] = rendered[i] + cover[parent[i]]."""
    nodes = h["nodes"]
    N = nodes.shape[0]
    rendered = torch.zeros(N, dtype=torch.int32, device=DEV)
    rendered[ri[:n].long()] = 1
    assert int(rendered.sum()) == n  # no node twice
    cover = rendered.clone()
    depth, parent = nodes[:, 0], nodes[:, 1].long()
    for d in range(1, int(depth.max()) + 1):
        lv = torch.nonzero(depth == d).flatten()
        cover[lv] += cover[parent[lv]]
    leaf = nodes[:, 3] > 0
    assert bool(torch.all(cover[leaf] == 1)), int((cover[leaf] != 1).sum())


@pytest.mark.parametrize("leaves,tau,log_scale,skybox", [(7_500_000, 3.0, -4.5, 20_000),
                                                         (37_500_000, 15.0, -6.0, 100_000)],
                         ids=["10M_tau3", "50M_tau15_bench"])
def test_config5_end_to_end_vs_oracle(leaves, tau, log_scale, skybox):
    """Config 5 (render_hierarchy.py:61-99): a synthetic merged hierarchy (10M nodes, tau = 3 px;
    and bench.py's full size: ~50M nodes, tau = 15 px, a ~7.4M-row cut), the cut seen from the
    camera -- bit-exact cut, parents, weights and child counts vs the oracle, every leaf covered
    once -- blended with the parents and rendered at 1920x1080 (forward, do_depth, no_grad)
    against the oracle's forward of the same rows (radii bit-exact, PSNR >= 137 dB)."""
    _config5_end_to_end_vs_oracle(leaves, tau, log_scale, skybox)


def _pose_hierarchy(h, pose):
    """The hierarchy's world stays where it was built (around the identity camera's frustum); the
    frame's camera becomes posed_cases.pose(pose)."""
    import posed_cases as PC
    p = PC.pose(pose, h["W"], h["H"])
    h.update(view=p["view"], proj=p["proj"], campos=p["campos"], tanfovx=p["tanfovx"], tanfovy=p["tanfovy"])
    return h


# tau = 40 px at 640x360: 2000 leaves give a cut of 1586 nodes (138 interior, 974 blended with their
# parents) of which 57 % reach the frame; 1000 leaves cannot keep 1000 nodes and an interior one
MILD = dict(leaves=2000, tau=40.0, log_scale=-3.5, skybox=200, W=640, H=360)


def test_config5_end_to_end_vs_oracle_mild_pose():
    """The same flow seen from a rotated, translated camera (posed_cases "mild": the cut's viewpoint
    is its campos, the blend's rows go through a view matrix that is no identity): the smallest
    hierarchy (in steps of 1000 leaves) whose cut keeps 1000 nodes, 30 % of them in the frame."""
    _config5_end_to_end_vs_oracle(MILD["leaves"], MILD["tau"], MILD["log_scale"], MILD["skybox"], W=MILD["W"],
                                  H=MILD["H"], pose="mild", min_cut=999, min_vis_share=0.3, sample=500)


def _config5_end_to_end_vs_oracle(leaves, tau, log_scale, skybox, W=1920, H=1080, pose=None, min_cut=1_000_000,
                                  min_vis_share=None, sample=20_000):
    import gs_oracle as O
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gs_train.hier import interpolate_cut
    from gs_train.synthetic import synthetic_lod_hierarchy, tau_threshold
    h = synthetic_lod_hierarchy(leaves, W, H, DEV, seed=5, skybox=skybox, log_scale_mean=log_scale)
    if pose:
        _pose_hierarchy(h, pose)
    N = h["nodes"].shape[0]
    assert N >= leaves * 4 // 3
    thr = float(np.float32(tau_threshold(tau, h["tanfovx"], W)))
    n, ri, pi, ni, w, k = _cut_hip(h, thr)
    assert min_cut < n < N
    # the cut against the oracle
    nodes_np, boxes_np = h["nodes"].cpu().numpy(), h["boxes"].cpu().numpy()
    ori, opi, oni = O.expand_to_size(nodes_np, boxes_np, np.float32(thr), h["campos"])
    np.testing.assert_array_equal(ri[:n].cpu().numpy(), ori)
    np.testing.assert_array_equal(pi[:n].cpu().numpy(), opi)
    np.testing.assert_array_equal(ni[:n].cpu().numpy(), oni)
    ow, ok = O.interpolation_weights(oni, np.float32(thr), nodes_np, boxes_np, np.asarray(h["campos"], np.float32))
    np.testing.assert_array_equal(w[:n].cpu().numpy(), ow)
    np.testing.assert_array_equal(k[:n].cpu().numpy(), ok)
    del nodes_np, boxes_np
    _covered_once(h, ri, n)
    S = h["skybox"]
    with torch.no_grad():
        m, sc, rot, op, sh = interpolate_cut(h["means3D"], h["scales"], h["rotations"], h["opacities"], h["shs"],
                                             ri[:n], pi, w, S)
    rows = n + S
    # blended rows vs the numpy restatement of render_post on a sample of rows
    smp = np.random.default_rng(0).choice(n, sample, replace=False)
    idx = np.concatenate([ori[smp], opi[smp][opi[smp] >= 0]])
    uniq, inv = np.unique(idx, return_inverse=True)
    take = lambda t: t[torch.tensor(uniq, device=DEV)].cpu().numpy()
    f = dict(xyz=take(h["means3D"]), scaling=take(h["scales"]), rotation=take(h["rotations"]),
             opacity=take(h["opacities"]), features=take(h["shs"]))
    loc_c = inv[:len(smp)]
    loc_p = np.where(opi[smp] >= 0, 0, -1)
    loc_p[opi[smp] >= 0] = inv[len(smp):]
    ref = hier_ref.interpolate_cut(f["xyz"], f["scaling"], f["rotation"], f["opacity"], f["features"], loc_c,
                                   np.where(loc_p < 0, loc_c, loc_p), w[:n].cpu().numpy()[smp], 0)
    for name, got in (("means3D", m), ("scales", sc), ("rotations", rot), ("opacities", op), ("shs", sh)):
        np.testing.assert_array_equal(got[torch.tensor(smp, device=DEV)].cpu().numpy(), ref[name], err_msg=name)
    # forward render of the cut vs the oracle
    t = lambda x: torch.tensor(x, dtype=torch.float32, device=DEV)
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=float(h["tanfovx"]), tanfovy=float(h["tanfovy"]), bg=t(bg),
        scale_modifier=1.0, viewmatrix=t(h["view"]).reshape(4, 4), projmatrix=t(h["proj"]).reshape(4, 4),
        sh_degree=3, campos=t(h["campos"]), prefiltered=False, debug=False, do_depth=True,
        render_indices=torch.empty(0, dtype=torch.int32), parent_indices=torch.empty(0, dtype=torch.int32),
        interpolation_weights=w, num_node_kids=k)
    with torch.no_grad():
        color, radii, invd = GaussianRasterizer(rs)(means3D=m, means2D=torch.zeros_like(m), shs=sh, opacities=op,
                                                    scales=sc, rotations=rot)
    torch.cuda.synchronize()
    cpu = lambda x: x.cpu().numpy()
    st = O.forward(cpu(m), cpu(op), h["view"], h["proj"], h["campos"], bg, W, H, h["tanfovx"], h["tanfovy"],
                   sh_degree=3, shs=cpu(sh), scales=cpu(sc), rotations=cpu(rot))
    np.testing.assert_array_equal(cpu(radii), st["radii"])
    assert rows == m.shape[0]
    if min_vis_share is None:
        assert int((radii > 0).sum()) > 1_000_000
    else:  # of the cut's own rows (the skybox rows follow them)
        assert int((radii[:n] > 0).sum()) >= min_vis_share * n, (int((radii[:n] > 0).sum()), n)
    p = psnr(cpu(color), st["color"])
    off = float(np.mean(np.abs(cpu(color) - st["color"]) > 1e-4))
    record_margins("config5_cut_forward" + ("_" + pose if pose else ""), psnr=p if np.isfinite(p) else 999.0, frac_off=off,
                   invdepth_rel_l2=float(np.linalg.norm(cpu(invd) - st["invdepth"]) / np.linalg.norm(st["invdepth"])))
    # ~10x from the observed 147.9 dB / no pixel off (profiles/r04_parity_margins.jsonl)
    assert p >= 137.0, p
    assert off <= 1e-6, off
    # the same frame through the rasterizer's own cut (render_indices: the blend fused into its
    # preprocess and colour pass -- at this size the colour pass forks ahead of the preprocess and
    # colours every row): bitwise the render_post-order frame above, as bench.py's config 5 runs it
    from diff_gaussian_rasterization import _C
    N = h["means3D"].shape[0]
    sky = torch.arange(N - S, N, dtype=torch.int32, device=DEV)
    ri2, pi2 = torch.cat([ri[:n], sky]), torch.cat([pi[:n], sky])
    w2 = torch.cat([w[:n], torch.ones(S, device=DEV)])
    e = torch.empty(0, device=DEV)
    with torch.no_grad():
        f = _C.rasterize_gaussians(t(bg), h["means3D"], e, h["opacities"], h["scales"], h["rotations"], 1.0, e,
                                   t(h["view"]).reshape(4, 4), t(h["proj"]).reshape(4, 4), float(h["tanfovx"]),
                                   float(h["tanfovy"]), H, W, h["shs"], 3, t(h["campos"]), False, False, ri2, pi2, w2, k,
                                   True, need_backward=False)
    torch.cuda.synchronize()
    assert torch.equal(f[1], color) and torch.equal(f[2], invd) and torch.equal(f[3], radii)  # K, colour, invdepth, radii


def test_rasterizer_render_indices_equal_render_post_blend():
    """Non-empty render_indices in the rasterizer (the blend done inside gsr_rasterize_forward)
    against render_post's order of work (interpolate_cut, then the rasterizer on the R rows):
    identical image / radii / K; gradients of the N hierarchy rows equal up to the order of the
    float atomics that sum shared parents; means2D's gradient in rows [0, R)."""
    from helpers import deterministic
    with deterministic():
        _render_indices_equal_render_post_blend()


def _render_indices_equal_render_post_blend():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gs_train.hier import interpolate_cut
    from gs_train.synthetic import synthetic_lod_hierarchy, tau_threshold
    W, H = 640, 360
    h = synthetic_lod_hierarchy(60_000, W, H, DEV, seed=9, zmin=1.0, zmax=12.0, log_scale_mean=-3.5)
    thr = tau_threshold(20.0, h["tanfovx"], W)
    n, ri, pi, ni, w, k = _cut_hip(h, thr)
    N = h["means3D"].shape[0]
    assert 0 < n < N
    t = lambda x: torch.tensor(x, dtype=torch.float32, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    gc = torch.randn(3, H, W, generator=g, device=DEV)
    gd = torch.randn(1, H, W, generator=g, device=DEV)

    def settings(ri_, pi_, w_):
        return GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=float(h["tanfovx"]), tanfovy=float(h["tanfovy"]),
            bg=t([0.3, 0.2, 0.1]), scale_modifier=1.0, viewmatrix=t(h["view"]).reshape(4, 4),
            projmatrix=t(h["proj"]).reshape(4, 4), sh_degree=3, campos=t(h["campos"]), prefiltered=False,
            debug=False, do_depth=True, render_indices=ri_, parent_indices=pi_, interpolation_weights=w_,
            num_node_kids=k)

    def leaves():
        return [h[x].detach().clone().requires_grad_(True) for x in ("means3D", "scales", "rotations", "opacities",
                                                                      "shs")]

    # (a) inside the rasterizer
    m, sc, rot, op, sh = leaves()
    m2a = torch.zeros(N, 3, device=DEV, requires_grad=True)
    ca, ra, da = GaussianRasterizer(settings(ri[:n], pi, w))(means3D=m, means2D=m2a, shs=sh, opacities=op,
                                                             scales=sc, rotations=rot)
    ((ca * gc).sum() + (da * gd).sum()).backward()
    ga = [x.grad for x in (m, sc, rot, op, sh)]
    # (b) render_post's order: blend, then rasterize the R rows
    m, sc, rot, op, sh = leaves()
    bm, bs, br, bo, bsh = interpolate_cut(m, sc, rot, op, sh, ri[:n], pi, w, 0)
    m2b = torch.zeros(n, 3, device=DEV, requires_grad=True)
    e = torch.empty(0, dtype=torch.int32)
    cb, rb, db = GaussianRasterizer(settings(e, e, torch.empty(0, device=DEV)))(
        means3D=bm, means2D=m2b, shs=bsh, opacities=bo, scales=bs, rotations=br)
    ((cb * gc).sum() + (db * gd).sum()).backward()
    gb = [x.grad for x in (m, sc, rot, op, sh)]
    assert torch.equal(ca, cb) and torch.equal(da, db) and torch.equal(ra, rb)
    assert ra.shape[0] == n
    for name, x, y in zip(("means3D", "scales", "rotations", "opacities", "shs"), ga, gb):
        err = float((x - y).norm() / y.norm().clamp_min(1e-30))
        assert err <= 1e-6, (name, err)
    assert torch.equal(m2a.grad[:n], m2b.grad) and int(m2a.grad[n:].abs().sum()) == 0


@pytest.mark.parametrize("skybox", [0, 3000])
def test_fused_cut_frame_equals_render_post_blend(skybox):
    """A no_grad frame with non-empty render_indices (render_hierarchy.py's evaluation) reads the cut's
    rows in place: render_post's blend fused into the preprocess and the SH colour pass, no R-row copy
    (gsr_device.h CutRef).  Against render_post's order of work (interpolate_cut, then the rasterizer
    on the R rows, skybox rows appended): image, inverse depth, radii and K bitwise equal.  The skybox
    rides in render_indices as rows with weight 1 (their own parent), as render_post blends them."""
    _fused_cut_frame_equals_render_post_blend(skybox)


def test_fused_cut_frame_equals_render_post_blend_mild_pose():
    """The same from a rotated, translated camera (posed_cases "mild"): the fused colour pass forms
    the SH direction from campos and recomputes the view depth through the view matrix."""
    _fused_cut_frame_equals_render_post_blend(3000, pose="mild")


def _fused_cut_frame_equals_render_post_blend(skybox, pose=None):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, _C
    from gs_train.hier import interpolate_cut
    from gs_train.synthetic import synthetic_lod_hierarchy, tau_threshold
    W, H = 1280, 720
    h = synthetic_lod_hierarchy(300_000, W, H, DEV, seed=11, zmin=1.0, zmax=25.0, log_scale_mean=-3.5, skybox=skybox)
    if pose:
        _pose_hierarchy(h, pose)
    thr = tau_threshold(12.0, h["tanfovx"], W)
    n, ri, pi, ni, w, k = _cut_hip(h, thr)
    N = h["means3D"].shape[0]
    assert 1000 < n < N
    S = h["skybox"]
    sky = torch.arange(N - S, N, dtype=torch.int32, device=DEV)
    ri2 = torch.cat([ri[:n], sky])
    pi2 = torch.cat([pi[:n], sky])
    w2 = torch.cat([w[:n], torch.ones(S, device=DEV)])
    t = lambda x: torch.tensor(x, dtype=torch.float32, device=DEV)
    rs = dict(bg=t([0.1, 0.2, 0.3]), viewmatrix=t(h["view"]).reshape(4, 4), projmatrix=t(h["proj"]).reshape(4, 4),
              campos=t(h["campos"]))
    e = torch.empty(0, device=DEV)
    with torch.no_grad():
        f = _C.rasterize_gaussians(rs["bg"], h["means3D"], e, h["opacities"], h["scales"], h["rotations"], 1.0, e,
                                   rs["viewmatrix"], rs["projmatrix"], float(h["tanfovx"]), float(h["tanfovy"]), H, W,
                                   h["shs"], 3, rs["campos"], False, False, ri2, pi2, w2, k, True, need_backward=False)
        bm, bs, br, bo, bsh = interpolate_cut(h["means3D"], h["scales"], h["rotations"], h["opacities"], h["shs"],
                                              ri[:n], pi, w, S)
        g = _C.rasterize_gaussians(rs["bg"], bm, e, bo, bs, br, 1.0, e, rs["viewmatrix"], rs["projmatrix"],
                                   float(h["tanfovx"]), float(h["tanfovy"]), H, W, bsh, 3, rs["campos"], False, False,
                                   None, None, None, None, True, need_backward=False)
        # the same cut in a frame a backward may follow: blended rows kept in its geometry buffer
        m = _C.rasterize_gaussians(rs["bg"], h["means3D"], e, h["opacities"], h["scales"], h["rotations"], 1.0, e,
                                   rs["viewmatrix"], rs["projmatrix"], float(h["tanfovx"]), float(h["tanfovy"]), H, W,
                                   h["shs"], 3, rs["campos"], False, False, ri2, pi2, w2, k, True, need_backward=True)
    torch.cuda.synchronize()
    assert f[0] == g[0] == m[0] > 0  # K
    for a_, b_, c_ in zip(f[1:4], g[1:4], m[1:4]):  # colour, inverse depth, radii
        assert torch.equal(a_, b_) and torch.equal(a_, c_)
    # no R-row copy in the fused frame's geometry buffer (59 floats per row in the other)
    assert f[4].numel() + 236 * (n + S) <= m[4].numel()


def test_expand_to_size_capacity_with_multi_gaussian_nodes():
    """A node can hold several Gaussians (count_leafs + count_merged > 1), so the cut can be longer
    than the node count N: output arrays of N entries are refused (the call fails; nothing is written
    past them), and arrays of the needed length get the full cut."""
    from gaussian_hierarchy._C import expand_to_size
    # root (1 merged Gaussian) with three leaf nodes of 3 Gaussians each; every box contains the
    # viewpoint, so every node is "too big" and renders its leaf Gaussians: 9 entries from 4 nodes
    nodes = torch.tensor([[0, -1, 0, 0, 1, 1, 3], [1, 0, 1, 3, 0, -1, 0], [1, 0, 4, 3, 0, -1, 0],
                          [1, 0, 7, 3, 0, -1, 0]], dtype=torch.int32, device=DEV)
    boxes = torch.zeros(4, 2, 4, device=DEV)
    boxes[:, 0, :3], boxes[:, 0, 3], boxes[:, 1, :3] = -10.0, 20.0, 10.0
    cam = torch.zeros(3, device=DEV)
    # 4-entry views of 12-entry buffers: the one pass writes the entries that fit, never past them
    room = [torch.full((12,), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    small = [t[:4] for t in room]
    with pytest.raises(RuntimeError, match="needs 9 entries"):
        expand_to_size(nodes, boxes, 0.01, cam, torch.zeros(3), *small)
    assert all(bool(torch.all(t[4:] == -7)) for t in room)
    big = [torch.full((12,), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
    n = expand_to_size(nodes, boxes, 0.01, cam, torch.zeros(3), *big)
    assert n == 9
    assert big[0][:9].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert big[1][:9].tolist() == [0] * 9  # the parent's first Gaussian
    assert big[2][:9].tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 3]
    assert all(bool(torch.all(t[9:] == -7)) for t in big)
