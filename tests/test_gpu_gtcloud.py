"""GPU tests of the ground-truth cloud constraint (csrc/gtcloud.hip, include/gsr_gtcloud.h,
gs_train.gtcloud): every mask bit for bit against the float32 all-pairs rule of tests/gt_ref.py;
densify_and_prune(gt_cloud=...) against the reference's own run with gt_point_cloud_constraints on
(tests/golden/densify_prune_gt_*.npz, made by tests/golden/make_gt_prune_golden.py); the chunk loop
with a cloud."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gt_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gpu_mask(cloud, thr, xyz, **kw):
    from gs_train.gtcloud import GtPointCloud
    c = GtPointCloud(cloud, threshold=thr, device=DEV)
    m = c.far_mask(torch.tensor(xyz, device=DEV), **kw)
    assert m.dtype == torch.bool and tuple(m.shape) == (xyz.shape[0],)
    out = m.cpu().numpy()
    c.close()
    return out


def _check(cloud, thr, xyz, what=""):
    want = gt_ref.far_mask(xyz, cloud, thr)
    got = _gpu_mask(cloud, thr, xyz)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {xyz.shape[0]} rows differ, first {bad[:5]}: {xyz[bad[:5]]}"
    return want


def _random_problem(thr, shift=(0.0, 0.0, 0.0), G=20_000, P=5000, seed=0):
    """G points in a 10 m box; P queries: four in ten a cloud point moved by up to 2 thr (near and far
    at every thr), a tenth outside the XY bounds, some exactly on a bound, some with a NaN or an Inf
    coordinate, the others anywhere in the box grown by a metre."""
    rng = np.random.default_rng(seed)
    shift = np.asarray(shift, np.float64)
    cloud = (rng.random((G, 3)) * 10.0 + shift).astype(np.float32)
    q = rng.random((P, 3)) * 12.0 - 1.0 + shift
    near = rng.random(P) < 0.4
    d = rng.normal(size=(P, 3))
    d *= (rng.random((P, 1)) * 2.0 * thr) / np.linalg.norm(d, axis=1, keepdims=True)
    q[near] = cloud[rng.integers(0, G, P)][near].astype(np.float64) + d[near]
    out = rng.random(P) < 0.1
    q[out, 0] += np.where(rng.random(out.sum()) < 0.5, -13.0, 13.0)
    q = q.astype(np.float32)
    x_min, x_max, y_min, y_max = gt_ref.bounds(cloud)
    q[0:40:4, 0], q[1:40:4, 0], q[2:40:4, 1], q[3:40:4, 1] = x_min, x_max, y_min, y_max
    q[40:44, 0], q[44:48, 1] = np.nextafter(x_min, -np.inf, dtype=np.float32), np.nextafter(y_max, np.inf,
                                                                                        dtype=np.float32)
    special = [np.nan, np.inf, -np.inf]
    for k, (col, v) in enumerate((c, v) for c in range(3) for v in special):
        q[50 + 3 * k:53 + 3 * k, col] = v
    return cloud, q


@pytest.mark.parametrize("thr", [0.05, 0.3, 2.0])
def test_random_cloud(thr):
    """thr far below, near and far above the mean spacing (0.37 m)."""
    cloud, q = _random_problem(thr)
    want = _check(cloud, thr, q, f"thr {thr}")
    inside = gt_ref.inside_bounds(q, cloud)
    assert (~inside).sum() > 300 and not want[~inside].any()
    assert inside[:40].sum() >= 20               # rows exactly on a bound are inside (inclusive) ...
    assert not inside[40:48].any()               # ... and one ulp outside they are not
    assert not want[50:71].any()                 # NaN / Inf x or y: outside; NaN z: no comparison holds
    assert np.array_equal(want[71:77], inside[71:77])  # an infinite z: every d2 is +Inf
    if thr < 2.0:
        assert 0.1 < want[inside].mean() < 0.9   # both decisions well represented


def test_large_coordinates():
    """The cloud and the queries shifted by (1e5, -2e5, 300): one fp32 step is 8 to 16 mm there, the
    cell coordinates are inexact, and the mask is still the all-pairs one."""
    cloud, q = _random_problem(0.05, shift=(1e5, -2e5, 300.0), seed=1)
    want = _check(cloud, 0.05, q, "shifted")
    inside = gt_ref.inside_bounds(q, cloud)
    assert 0.05 < want[inside].mean() < 0.95


def test_lattice_ties():
    """Coordinates on the 1/64 lattice and thr = 0.25 = 16/64: every d2 is exact in fp32 whatever
    the formulation, so ties are ties.  A query exactly 0.25 from its only near point is not far
    (d2 > thr^2 fails); one lattice step farther it is."""
    s = 1.0 / 64.0
    ax = np.arange(0.0, 10.5, 2.0)
    cloud = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    inner = cloud[np.all((cloud >= 2) & (cloud <= 8), 1)]
    offs, want = [], []
    for k in range(3):
        for sign in (-1.0, 1.0):
            for steps, far in ((16, False), (17, True), (15, False)):
                o = np.zeros(3)
                o[k] = sign * steps * s
                offs.append(o)
                want.append(far)
    for o, far in (((12, 10, 3), False), ((12, 10, 4), True), ((-9, 9, -9), False), ((10, -10, 8), True),
                   ((0, 0, 0), False)):
        offs.append(np.array(o) * s)
        want.append(far)
    q = (inner[:, None, :] + np.array(offs)[None]).reshape(-1, 3).astype(np.float32)
    want = np.tile(np.array(want), inner.shape[0])
    assert np.array_equal(gt_ref.far_mask(q, cloud, 0.25), want)  # the reference agrees with the arithmetic
    assert np.array_equal(_gpu_mask(cloud, 0.25, q), want)


def test_sizes_and_degenerate_extents():
    """G around a wave's width, P of zero, one and just over a wave, a cloud of identical points
    (zero extent: the XY bounds are one point) and a cloud on one plane."""
    rng = np.random.default_rng(5)
    thr = 0.2

    def queries(cloud, P):
        base = cloud[rng.integers(0, cloud.shape[0], P)].astype(np.float64)
        q = base + rng.normal(size=(P, 3)) * 0.15
        keep = rng.random(P) < 0.5  # exactly above / below a cloud point (the only way inside when G = 1)
        q[keep, :2] = base[keep, :2]
        q[keep, 2] = base[keep, 2] + rng.choice([0.0, 0.1, thr, 0.4, -0.4], keep.sum())
        return q.astype(np.float32)
    for G in (1, 63, 64, 65):
        cloud = (rng.random((G, 3)) * 2.0).astype(np.float32)
        for P in (0, 1, 65):
            want = _check(cloud, thr, queries(cloud, P), f"G {G} P {P}")
            assert want.shape == (P,)
    same = np.tile(np.array([[1.5, -2.25, 3.0]], np.float32), (100, 1))
    want = _check(same, thr, queries(same, 200), "identical points")
    assert want.any() and not want.all()
    plane = (rng.random((500, 3)) * 4.0).astype(np.float32)
    plane[:, 2] = 0.75
    want = _check(plane, thr, queries(plane, 300), "one plane")
    assert want.any() and not want.all()
    for axis in (0, 1):
        line = (rng.random((300, 3)) * 4.0).astype(np.float32)
        line[:, axis] = -1.0
        _check(line, thr, queries(line, 200), f"zero extent along axis {axis}")


def test_one_crowded_cell():
    """50 000 points inside a 1 cm cube (a scanner's own position) and 2000 scattered ones: the wave
    shares the long run; queries around both."""
    rng = np.random.default_rng(9)
    thr = 0.05
    cube = (np.array([5.0, 5.0, 5.0]) + rng.random((50_000, 3)) * 0.01).astype(np.float32)
    scat = (rng.random((2000, 3)) * 10.0).astype(np.float32)
    cloud = np.concatenate([scat[:1000], cube, scat[1000:]])
    qa = np.array([5.005, 5.005, 5.005]) + (rng.random((1200, 3)) - 0.5) * 0.12
    d = rng.normal(size=(800, 3))
    d *= (rng.random((800, 1)) * 2.0 * thr) / np.linalg.norm(d, axis=1, keepdims=True)
    qb = scat[rng.integers(0, 2000, 800)] + d
    q = np.concatenate([qa, qb, rng.random((200, 3)) * 10.0]).astype(np.float32)
    want = _check(cloud, thr, q, "crowded cell")
    assert 0.2 < want[:1200].mean() < 0.95 and 0.2 < want[1200:2000].mean() < 0.8


def one_cell_problem(G, thr=0.25):
    """G points inside a cube of side thr / 2 (below the cell edge: one cell, one run of G points in
    input order) and three sets of 65 queries, a second wave of one lane each.  Rows 1 .. G - 2 lie in
    the cube's lowest layer, row 0 in its low corner's opposite XY corner at the bottom, the last row at
    the top centre: it alone is within thr of a query 0.9 thr above it, so whoever finds a point has
    read the end of the run.  [0]: by row % 4 such a query (rows 0 and 3 mod 4), one 3 thr above the
    cube (no point in reach along z: no search) and one 0.95 thr below the corner (x_min, y_min) (it
    walks the whole run and stays far).  [1] .. [4]: row 0 / row 63 alone inside the XY bounds, above the
    last point or below the corner: the owner of the wave's run at either end of the wave."""
    rng = np.random.default_rng(400 + G)
    o, s = np.array([1.0, 2.0, 3.0]), thr / 2
    cloud = o + rng.random((G, 3)) * [s, s, 0.05 * thr] + [0.0, 0.0, 0.1 * thr]
    cloud[0] = o + [s, s, 0.0]
    cloud[1] = o + [0.0, 0.0, 0.1 * thr]
    cloud[G - 1] = o + [s / 2, s / 2, s]
    above = o + np.concatenate([rng.random((65, 2)) * s, np.full((65, 1), s + 0.9 * thr)], 1)
    high = above + [0.0, 0.0, 2.1 * thr]
    below = np.tile(o + [0.0, 0.0, -0.95 * thr], (65, 1))
    kind = np.arange(65) % 4
    mixed = np.where((kind == 1)[:, None], high, np.where((kind == 2)[:, None], below, above))
    sets = [mixed]
    for lane in (0, 63):
        for src in (above, below):
            q = mixed + [-1.0, 0.0, 0.0]  # outside the XY bounds
            q[lane] = src[lane]
            sets.append(q)
    return cloud.astype(np.float32), [q.astype(np.float32) for q in sets]


@pytest.mark.parametrize("G", [16, 17, 64, 65, 129])
def test_one_cell_run_lengths_and_the_owner_broadcast(G):
    """One cell holding one run of G points, G on either side of the lane / wave split and of a
    64-point slice, with the only point within thr at the run's end, so an early exit cannot hide a
    slice that was not read; the wave's run owned by lane 0 and by lane 63."""
    from gs_train.gtcloud import GtPointCloud
    thr = 0.25
    cloud, sets = one_cell_problem(G, thr)
    c = GtPointCloud(cloud, threshold=thr, device=DEV)
    try:
        assert c.cells == 1 and c.G == G  # the run length is G
        for k, q in enumerate(sets):
            want = gt_ref.far_mask(q, cloud, thr)
            inside = gt_ref.inside_bounds(q, cloud)
            if k == 0:
                assert inside.all() and np.array_equal(want, np.arange(65) % 4 % 3 != 0)  # both decisions
            else:
                lane = (0, 0, 63, 63)[k - 1]
                assert np.array_equal(np.nonzero(inside)[0], [lane]) and want[lane] == (k % 2 == 0)
            got = c.far_mask(torch.tensor(q, device=DEV)).cpu().numpy()
            assert np.array_equal(got, want), (G, k, np.nonzero(got != want)[0])
    finally:
        c.close()


def test_far_mask_with_existing_and_protected_masks():
    cloud, q = _random_problem(0.3, seed=3)
    rng = np.random.default_rng(4)
    existing, protected = rng.random(q.shape[0]) < 0.3, rng.random(q.shape[0]) < 0.3
    te, tp = torch.tensor(existing, device=DEV), torch.tensor(protected, device=DEV)
    far = gt_ref.far_mask(q, cloud, 0.3)
    assert (far & existing).any() and (far & protected & ~existing).any()
    for e, p, ke, kp in ((existing, protected, te, tp), (existing, None, te, None), (None, protected, None, tp)):
        want = gt_ref.compare_points_to_gt(q, cloud, 0.3, e, p)
        got = _gpu_mask(cloud, 0.3, q, existing_mask=ke, protected_mask=kp)
        assert np.array_equal(got, want)
    # the reference's combination, spelled out
    want = existing | (far & ~existing & ~protected)
    assert np.array_equal(_gpu_mask(cloud, 0.3, q, existing_mask=te, protected_mask=tp), want)


def test_cloud_reports_bounds_and_memory():
    from gs_train.gtcloud import GtPointCloud
    cloud, _ = _random_problem(0.05, seed=6)
    c = GtPointCloud(torch.tensor(cloud, device=DEV), threshold=0.05)
    assert (c.x_min, c.x_max, c.y_min, c.y_max) == gt_ref.bounds(cloud)
    assert c.G == cloud.shape[0] and 1 <= c.cells <= c.G
    assert c.bytes == 16 * c.G + 12 * c.cells + 4  # 16 B per point, 12 B per occupied cell
    with pytest.raises(ValueError):
        GtPointCloud(np.array([[0.0, np.nan, 0.0]], np.float32), device=DEV)
    with pytest.raises(ValueError):
        GtPointCloud(np.zeros((0, 3), np.float32), device=DEV)
    c.close()
    with pytest.raises(RuntimeError):
        c.far_mask(torch.zeros(1, 3, device=DEV))


# ---- densify_and_prune with the cloud against the reference's own run -------------------------

def _fixture_model(d):
    from gs_train import Adam
    from gs_train.harness import GaussianSet
    t = lambda k: torch.tensor(d[k], device=DEV).contiguous()
    P = d["in_xyz"].shape[0]
    g = GaussianSet(means3D=np.zeros((P, 3), np.float32), shs=np.zeros((P, 16, 3), np.float32),
                    opacities=np.full((P, 1), 0.5, np.float32), scales=np.ones((P, 3), np.float32),
                    rotations=np.zeros((P, 4), np.float32), device=DEV, joined_features=True)
    with torch.no_grad():  # the raw parameters exactly as the reference held them
        g._xyz.copy_(t("in_xyz"))
        g._features.copy_(torch.cat((t("in_f_dc"), t("in_f_rest")), 1))
        g._opacity.copy_(t("in_opacity"))
        g._scaling.copy_(t("in_scaling"))
        g._rotation.copy_(t("in_rotation"))
    g.xyz_gradient_accum, g.max_radii2D, g.denom = t("in_accum"), t("in_max_radii2D"), t("in_denom")
    opt = Adam(g.param_groups(), lr=0.0, eps=1e-15)
    mom = {"_xyz": ("xyz",), "_features": ("f_dc", "f_rest"), "_opacity": ("opacity",), "_scaling": ("scaling",),
           "_rotation": ("rotation",)}
    for name, keys in mom.items():
        opt.state[getattr(g, name)] = {"step": torch.tensor(7.0),
                                       "exp_avg": torch.cat([t("in_m_" + k) for k in keys], 1),
                                       "exp_avg_sq": torch.cat([t("in_v_" + k) for k in keys], 1)}
    return g, opt, mom


@pytest.mark.parametrize("case", ["plain", "scaffold"])
def test_densify_and_prune_with_cloud_matches_reference_run(case):
    """The comparisons of test_gpu_densify.test_densify_and_prune_matches_reference_run, on the
    reference's run with gt_point_cloud_constraints on; the inputs are densify_prune_<case>.npz's."""
    from gs_train.densify import densify_and_prune
    from gs_train.gtcloud import GtPointCloud
    d = dict(np.load(os.path.join(GOLD, f"densify_prune_{case}.npz")))
    d.update(np.load(os.path.join(GOLD, f"densify_prune_gt_{case}.npz")))
    t = lambda k: torch.tensor(d[k], device=DEV).contiguous()
    g, opt, mom = _fixture_model(d)
    P = g.P
    cloud = GtPointCloud(d["cloud"], threshold=float(d["threshold"]), device=DEV)
    assert np.array_equal(np.array([cloud.x_min, cloud.x_max, cloud.y_min, cloud.y_max], np.float32), d["bounds"])
    c = densify_and_prune(g, opt, float(d["max_grad"]), float(d["min_opacity"]), float(d["extent"]),
                          float(d["percent_dense"]), first_row=int(d["scaffold"]), normals=t("normals"),
                          gt_cloud=cloud)
    n = d["out_xyz"].shape[0]
    assert c["total"] == n and c["cloned"] > 0 and c["split"] > 0 and c["kept"] < P
    assert 2 * c["split"] == d["normals"].shape[0]
    assert c["gt_pruned"] == int(d["gt_pruned"]) > 0
    assert c["gt_pruned_fixed"] == int(d["gt_pruned_fixed"])
    assert (c["gt_pruned_fixed"] > 0) == (case == "scaffold")
    got = {"f_dc": g._features[:, :1], "f_rest": g._features[:, 1:], "opacity": g._opacity, "rotation": g._rotation}
    for k, v in got.items():
        np.testing.assert_array_equal(v.detach().cpu().numpy(), d["out_" + k], err_msg=k)
    old = c["kept"] + c["cloned"]  # rows before the split children: copies
    sc = g._scaling.detach().cpu().numpy()
    np.testing.assert_array_equal(sc[:old], d["out_scaling"][:old])
    np.testing.assert_allclose(sc, d["out_scaling"], rtol=4e-7, atol=0)  # as in test_gpu_densify
    xyz = g._xyz.detach().cpu().numpy()
    np.testing.assert_array_equal(xyz[:old], d["out_xyz"][:old])
    np.testing.assert_allclose(xyz, d["out_xyz"], rtol=1e-6, atol=1e-6)
    for name, keys in mom.items():
        st = opt.state[getattr(g, name)]
        for sk, pre in (("exp_avg", "out_m_"), ("exp_avg_sq", "out_v_")):
            want = np.concatenate([d[pre + k] for k in keys], 1)
            np.testing.assert_array_equal(st[sk].cpu().numpy(), want, err_msg=f"{name} {sk}")
        assert float(st["step"]) == 7.0
    np.testing.assert_array_equal(g.xyz_gradient_accum.cpu().numpy(), d["out_accum"])
    np.testing.assert_array_equal(g.denom.cpu().numpy(), d["out_denom"])
    np.testing.assert_array_equal(g.max_radii2D.cpu().numpy(), d["out_max_radii2D"])


def test_without_cloud_the_counts_have_no_new_keys():
    from gs_train.densify import densify_and_prune
    d = np.load(os.path.join(GOLD, "densify_prune_plain.npz"))
    g, opt, _ = _fixture_model(d)
    c = densify_and_prune(g, opt, float(d["max_grad"]), float(d["min_opacity"]), float(d["extent"]),
                          float(d["percent_dense"]), normals=torch.tensor(d["normals"], device=DEV), gt_cloud=None)
    assert set(c) == {"kept", "cloned", "split", "total"}


# ---- the chunk loop ---------------------------------------------------------------------------

def test_chunk_loop_prunes_against_the_cloud():
    """A small synthetic street chunk with its cloud through train_single.py's loop: three densify
    events.  Right after each, every row inside the cloud's XY bounds that is not one of the event's
    split children has a cloud point within the threshold; the counts add up against the
    unconstrained plan of the same rows (gsr_densify_plan changes nothing)."""
    from gs_train._native import lib, ptr, stream
    from gs_train.chunk import ChunkSchedule, TrainChunk, street_chunk
    from gs_train.native_step import NativeTrainStep
    n_it, thr = 130, 0.15
    torch.manual_seed(0)
    ts, info = street_chunk(NativeTrainStep, W=128, H=128, positions=6, faces=4, n_truth=20_000, n_init=6000,
                            skybox=200, n_scaffold=500, iterations=n_it, device=DEV, gt_cloud_points=8000,
                            gt_threshold=thr)
    cloud = info["gt_cloud"]
    assert ts.gt_cloud is cloud and cloud.threshold == thr and cloud.G == 8000
    cloud_np = info["gt_points"]
    assert cloud_np.shape == (8000, 3) and cloud_np.dtype == np.float32
    assert (cloud.x_min, cloud.x_max, cloud.y_min, cloud.y_max) == gt_ref.bounds(cloud_np)
    sched = ChunkSchedule(iterations=n_it, densification_interval=30, opacity_reset_interval=1000,
                          densify_from_iter=30, densify_until_iter=n_it, sh_interval=50,
                          densify_grad_threshold=0.0008, percent_dense=0.01)
    seen = []
    real = ts.densify_and_prune

    def recording(max_grad, min_opacity, percent_dense, normals=None):
        g = ts.g
        L = lib()
        scratch = torch.empty(max(1, L.gsr_densify_scratch_bytes(g.P)), dtype=torch.uint8, device=DEV)
        counts = torch.zeros(4, dtype=torch.int64, device=DEV)
        acc = g.xyz_gradient_accum.reshape(-1).contiguous()
        rc = L.gsr_densify_plan(g.P, ts.scaffold, ptr(acc), ptr(g.max_radii2D.contiguous()), ptr(g._opacity.detach()),
                                ptr(g._scaling.detach()), float(max_grad), float(min_opacity),
                                float(percent_dense * ts.extent), ptr(scratch), ptr(counts), stream(g._xyz.device))
        assert rc == 0
        plain = [int(v) for v in counts.cpu()]
        c = real(max_grad, min_opacity, percent_dense, normals=normals)
        seen.append((plain, dict(c), g._xyz.detach().cpu().numpy().copy()))
        return c
    ts.densify_and_prune = recording
    tc = TrainChunk(ts, sched)
    tc.run()
    torch.cuda.synchronize()
    dens = [e for e in tc.events if "total" in e]
    assert [e["iteration"] for e in dens] == [60, 90, 120] and len(seen) == 3
    for e, (plain, c, xyz) in zip(dens, seen):
        assert e["gt_pruned"] == c["gt_pruned"] and e["gt_pruned_fixed"] == c["gt_pruned_fixed"]
        assert e["P_after"] == c["total"] == xyz.shape[0]
        kept_u, cloned_u, split_u, total_u = plain
        assert c["split"] == split_u
        assert kept_u + cloned_u == c["kept"] + c["cloned"] + c["gt_pruned"]
        assert total_u - c["total"] == c["gt_pruned"]
        assert 0 <= c["gt_pruned_fixed"] <= c["gt_pruned"] and c["kept"] + c["split"] <= e["P_before"]
        rows = xyz[:c["kept"] + c["cloned"]]  # the children follow, never distance-tested
        assert not gt_ref.far_mask(rows, cloud_np, thr).any()
    assert any(c["gt_pruned"] > 0 for _, c, _ in seen)

