"""GPU tests of the LiDAR preparation (gs_train.lidar, csrc/lidar.hip) against tests/lidar_ref.py on the
cases of tests/lidar_cases.py: the mask exactly (tests/test_lidar_cpu.py holds the cases to the
condition that makes that a fair demand), the voxels, their order and counts exactly and the means
within 1 fp32 ulp, the chunk's cloud end to end, and the error paths."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import lidar_cases as C
import lidar_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _box_of(case):
    """The case's own crop box, or one that cuts through its points."""
    if case["box"] is not None:
        return case["box"]
    p = case["points"][np.isfinite(case["points"]).all(1)]
    if len(p) == 0:
        return (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    lo, hi = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
    return tuple((lo + hi) / 2 + 0.01), tuple(np.maximum((hi - lo) * 0.6, 0.05))


@pytest.mark.parametrize("name", C.MESH_CASES)
def test_near_mask_equals_the_float64_mask(name):
    from gs_train.lidar import MeshIndex, crop_bounds
    c = C.mesh_case(name)
    d2 = C.mesh_case_d2(name)
    index = MeshIndex(c["vertices"], c["faces"], max_distance=C.MAX_DISTANCE, device=DEV)
    try:
        info = index.info()
        assert info["vertices"] == len(c["vertices"]) and info["triangles"] == len(c["faces"])
        assert info["references"] + info["oversize"] >= 1 and info["bytes"] >= 36 * (info["references"] + info["oversize"])
        if name == "oversize":
            assert info["oversize"] == 2
        if name == "fan":
            assert info["references"] / max(info["cells"], 1) > 64  # the wave's path
        pts = _t(c["points"])
        center, extent = _box_of(c)
        assert np.array_equal(crop_bounds(center, extent), R.crop_bounds(center, extent))
        for box in (None, crop_bounds(center, extent)):
            for q in C.QUERY_DISTANCES:
                got = index.near_mask(pts, box=box, max_distance=q).cpu().numpy()
                want = R.near_mask(c["points"], d2, q, box)
                bad = np.nonzero(got != want)[0]
                assert len(bad) == 0, (name, q, box is not None, bad[:8], np.sqrt(d2[bad[:8]]))
    finally:
        index.close()


@pytest.mark.parametrize("F", C.ONE_CELL_COUNTS)
def test_one_cell_run_lengths_and_the_owner_broadcast(F):
    """One cell holding one run of F references, F on either side of the lane / wave split and of a
    64-reference slice, with the only triangle in reach at the run's end; the owner of the wave's run in
    lane 0 and in lane 63, and a second wave of one lane (tests/lidar_cases.py one_cell_case)."""
    from gs_train.lidar import MeshIndex
    c = C.one_cell_case(F)
    index = MeshIndex(c["vertices"], c["faces"], max_distance=C.MAX_DISTANCE, device=DEV)
    try:
        info = index.info()
        assert info["cells"] == 1 and info["references"] == F
        for k, pts in enumerate(c["points"]):
            d2 = R.min_d2(pts, c["vertices"], c["faces"], np.float64)
            for q in C.QUERY_DISTANCES:
                want = R.near_mask(pts, d2, q)
                assert want.any() and not want.all()  # the reference makes both decisions
                got = index.near_mask(_t(pts), max_distance=q).cpu().numpy()
                bad = np.nonzero(got != want)[0]
                assert len(bad) == 0, (F, k, q, bad[:8], np.sqrt(d2[bad[:8]]))
    finally:
        index.close()


def test_threshold_is_inclusive_on_an_exact_tie():
    """max_distance = 0.125 and points at exactly that distance from the face, an edge and a vertex of
    a triangle with power-of-two coordinates: every fp32 operation of the rule is exact, d2 = T."""
    from gs_train.lidar import MeshIndex
    c = C.TIE_CASE
    index = MeshIndex(c["vertices"], c["faces"], max_distance=C.TIE_DISTANCE, device=DEV)
    got = index.near_mask(_t(c["points"])).cpu().numpy()
    index.close()
    assert np.array_equal(got, C.TIE_EXPECTED)


def test_crop_alone_without_a_mesh():
    from gs_train.lidar import prepare_chunk_cloud
    c = C.mesh_case("placement")
    center, extent = c["box"]
    out = prepare_chunk_cloud(_t(c["points"]), None, center, extent, mesh=None, lidar_init=False)
    want = R.crop_mask(c["points"], R.crop_bounds(center, extent)) & np.isfinite(c["points"]).all(1)
    assert np.array_equal(out.points.cpu().numpy(), c["points"][want])
    assert out.colors is None and out.init_points is None and out.init_colors_u8 is None


@pytest.mark.parametrize("name", C.VOXEL_CASES)
def test_voxel_downsample_against_the_float64_mean(name):
    from gs_train.lidar import voxel_downsample
    pts, col, s = C.voxel_case(name)
    means, cmeans, counts, _ = R.voxel_mean(pts, col, s)
    p, c = _t(pts), (_t(col) if col is not None else None)
    xyz, rgb, cnt = voxel_downsample(p, c, s)
    assert np.array_equal(cnt.cpu().numpy(), counts)  # the same voxels, in ascending (iz, iy, ix) order
    assert R.ulp_diff(xyz.cpu().numpy(), means).max() <= 1  # row by row: the order is part of it
    if col is None:
        assert rgb is None
    else:
        assert R.ulp_diff(rgb.cpu().numpy(), cmeans).max() <= 1
    xyz2, rgb2, cnt2 = voxel_downsample(p, c, s)
    assert torch.equal(xyz, xyz2) and torch.equal(cnt, cnt2) and (rgb is None or torch.equal(rgb, rgb2))


def test_voxel_sums_run_in_input_order():
    """Three points of one voxel whose fp64 sum depends on the order: 2^60, 1 (absorbed), -2^60 in
    input order give 0, any other order 1/3.  The sort is stable and a short voxel is summed by one
    lane front to back, which is what makes two runs (and two machines) agree."""
    from gs_train.lidar import voxel_downsample
    big = float(2 ** 60)
    pts = np.array([[big, 0, 0], [1.0, 0, 0], [-big, 0, 0]], np.float32)
    xyz, _, cnt = voxel_downsample(_t(pts), None, float(2 ** 63))
    assert cnt.tolist() == [3] and xyz.cpu().numpy()[0].tolist() == [0.0, 0.0, 0.0]
    xyz, _, cnt = voxel_downsample(_t(pts[[0, 2, 1]]), None, float(2 ** 63))
    assert cnt.tolist() == [3] and xyz.cpu().numpy()[0, 0] == np.float32(1.0 / 3.0)


def test_voxel_mean_keep_mask_and_rejections():
    from gs_train import lidar
    pts, col, s = C.voxel_case("street")
    keep = np.random.default_rng(3).random(len(pts)) < 0.4
    means, cmeans, counts, _ = R.voxel_mean(pts[keep], col[keep], s)
    xyz, rgb, cnt = lidar._voxel_mean(_t(pts), _t(col), _t(keep.astype(np.uint8)), s)
    assert np.array_equal(cnt.cpu().numpy(), counts)
    assert R.ulp_diff(xyz.cpu().numpy(), means).max() <= 1 and R.ulp_diff(rgb.cpu().numpy(), cmeans).max() <= 1
    none = lidar._voxel_mean(_t(pts), None, _t(np.zeros(len(pts), np.uint8)), s)
    assert none[0].shape == (0, 3) and none[1] is None and none[2].shape == (0,)
    empty = lidar.voxel_downsample(torch.zeros((0, 3), device=DEV), None, s)
    assert empty[0].shape == (0, 3)
    rp, rs = C.REJECTED_VOXEL
    with pytest.raises(RuntimeError, match="2\\^31 - 1 voxels"):
        lidar.voxel_downsample(_t(rp), None, rs)
    bad = pts[:8].copy()
    bad[3, 1] = np.nan
    with pytest.raises(RuntimeError, match="NaN or Inf"):
        lidar.voxel_downsample(_t(bad), None, s)


def test_prepare_chunk_cloud_end_to_end(tmp_path):
    """3000 survey points over a terrain: crop, filter, chunk.ply, the initial points into the model."""
    from gs_train.gtcloud import GtPointCloud
    from gs_train.lidar import MeshIndex, prepare_chunk_cloud, voxel_downsample
    from gs_train.model_init import create_from_cloud
    rng = np.random.default_rng(12)
    v, f = C._terrain(20, 14, 0.3, rng)
    pts = C._around(v, f, 3000, rng)
    col = rng.uniform(0, 1, (3000, 3)).astype(np.float32)
    center, extent = (3.0, 2.0, 0.0), (4.0, 3.0, 10.0)
    mesh = MeshIndex(v, f, device=DEV)
    out = prepare_chunk_cloud(_t(pts), _t(col), center, extent, mesh=mesh, max_distance=0.1, density=2000)
    mesh.close()
    d2 = R.min_d2(pts, v, f)  # as the cases: no point within GUARD of the threshold
    keep = R.near_mask(pts, d2, 0.1, R.crop_bounds(center, extent))
    assert 300 < keep.sum() < 2700
    assert np.array_equal(out.points.cpu().numpy(), pts[keep]) and np.array_equal(out.colors.cpu().numpy(), col[keep])
    s = (1.0 / 2000) ** (1 / 3)
    means, cmeans, counts, _ = R.voxel_mean(pts[keep], col[keep], s)
    assert out.init_points.shape == means.shape and R.ulp_diff(out.init_points.cpu().numpy(), means).max() <= 1
    u8 = out.init_colors_u8.cpu().numpy()
    assert u8.dtype == np.uint8 and u8.shape == means.shape
    _, rgb, cnt = voxel_downsample(out.points, out.colors, s)  # bitwise what prepare_chunk_cloud computed
    assert np.array_equal(cnt.cpu().numpy(), counts) and R.ulp_diff(rgb.cpu().numpy(), cmeans).max() <= 1
    assert np.array_equal(u8, (rgb.cpu().numpy().astype(np.float64) * 255).astype(np.uint8))  # truncated
    path = tmp_path / "chunk.ply"
    out.save_ply(str(path))
    cloud = GtPointCloud.from_ply(str(path), threshold=0.05, device=DEV)
    from gs_train.gtcloud import read_ply_xyz
    assert np.array_equal(read_ply_xyz(str(path)), pts[keep]) and cloud.G == int(keep.sum())
    cloud.close()
    g, skybox, scaffold_points = create_from_cloud(out.init_points, out.init_colors_u8.float() / 255.0, n_images=4,
                                                   spatial_lr_scale=1.0)
    assert g.P == len(means) and scaffold_points is None
    off = prepare_chunk_cloud(_t(pts), _t(col), center, extent, mesh=None, lidar_init=False)
    assert off.init_points is None and off.init_colors_u8 is None
    assert np.array_equal(off.points.cpu().numpy(), pts[R.crop_mask(pts, R.crop_bounds(center, extent))])


def test_error_paths():
    from gs_train.lidar import MeshIndex
    c = C.mesh_case("sizes_P64_F2")
    v = c["vertices"].copy()
    v[1, 2] = np.inf
    with pytest.raises(RuntimeError, match="NaN or Inf"):
        MeshIndex(v, c["faces"], device=DEV)
    v[1, 2] = np.nan
    with pytest.raises(RuntimeError, match="NaN or Inf"):
        MeshIndex(v, c["faces"], device=DEV)
    for bad in (len(c["vertices"]), -1):
        f = c["faces"].copy()
        f[1, 2] = bad
        with pytest.raises(RuntimeError, match="out of range"):
            MeshIndex(c["vertices"], f, device=DEV)
    with pytest.raises(ValueError):
        MeshIndex(c["vertices"], c["faces"], max_distance=0.0, device=DEV)
    index = MeshIndex(c["vertices"], c["faces"], device=DEV)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        index.near_mask(torch.from_numpy(c["points"]))
    with pytest.raises(ValueError):
        index.near_mask(_t(c["points"]).double())
    index.close()
    with pytest.raises(RuntimeError, match="released"):
        index.near_mask(_t(c["points"]))
