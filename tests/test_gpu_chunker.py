"""GPU tests of the scene partition (gs_train.chunker, csrc/chunker.hip) against the per-chunk rule of
tests/chunker_ref.py on the cases of tests/chunker_cases.py.  Every decision is a strict comparison of
stored values, so everything is held to equality: the cells, the counts, the candidate list, the
chunks with their cameras after the seeded draws, the kept observations, the point rows and their
order, the depth cameras, center and extent."""
from __future__ import annotations

import random

import numpy as np
import pytest
import torch

import chunker_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _run(case, run, **kw):
    from gs_train.chunker import partition_scene
    return partition_scene(case["cam_centers"], case["obs_ptr"], case["obs_point_id"], case["point_id"],
                           case["point_xyz"], case["point_error"], depth_centers=case["depth_centers"],
                           chunk_size=case["chunk_size"], min_n_cams=run[0], max_n_cams=run[1], add_far_cams=run[2],
                           device=DEV, grid=case["grid"], **kw)


def _np(t):
    return t.cpu().numpy()


def _assert_equal(part, ref, what):
    for k in ("cell32", "cell64", "n_pts", "total", "blend"):
        got = _np(getattr(part, k))
        assert got.dtype == ref[k].dtype and np.array_equal(got, ref[k]), (what, k, np.argwhere(got != ref[k])[:8])
    assert np.array_equal(part.candidates, ref["candidates"]), (what, "candidates")
    assert part.excluded == ref["excluded"], (what, "excluded")
    assert [(c.i, c.j) for c in part.chunks] == [(c["i"], c["j"]) for c in ref["chunks"]], (what, "chunks")
    for got, want in zip(part.chunks, ref["chunks"]):
        tag = (what, got.i, got.j)
        assert np.array_equal(got.cameras, want["cameras"]), (tag, "cameras")
        offsets = np.concatenate([[0], np.cumsum([len(o) for o in want["obs"]])])
        assert np.array_equal(got.obs_offsets, offsets), (tag, "obs_offsets")
        flat = np.concatenate(want["obs"] + [np.zeros(0, np.int64)])
        assert got.obs_index.dtype == torch.int64 and np.array_equal(_np(got.obs_index), flat), (tag, "obs_index")
        assert np.array_equal(_np(got.points), want["points"]), (tag, "points")
        assert np.array_equal(got.blend, want["blend"]), (tag, "blend")
        assert np.array_equal(got.depth_cameras, want["depth_cameras"]), (tag, "depth_cameras")
        assert got.center.dtype == np.float64 and np.array_equal(got.center, want["center"]), (tag, "center")
        assert got.extent.dtype == np.float64 and np.array_equal(got.extent, want["extent"]), (tag, "extent")


@pytest.mark.parametrize("name", list(C.cases()))
def test_partition_equals_the_per_chunk_rule(name):
    case = C.cases()[name]
    for run in case["runs"]:
        part = _run(case, run)
        g = C.grid_of(case)
        assert (part.n_w, part.n_h) == (g[1], g[2]) and np.array_equal(part.global_bbox, g[0])
        _assert_equal(part, C.reference(name, run), (name, run))


def test_inputs_already_on_the_device_and_a_callers_generator():
    from gs_train.chunker import partition_scene
    import chunker_ref as R
    case = C.cases()["auto"]
    t = {k: torch.from_numpy(case[k]).to(DEV) for k in ("obs_point_id", "point_id", "point_xyz", "point_error")}
    part = partition_scene(case["cam_centers"], case["obs_ptr"], t["obs_point_id"], t["point_id"], t["point_xyz"],
                           t["point_error"], depth_centers=case["depth_centers"], max_n_cams=6, rng=random.Random(1234),
                           device=DEV)
    ref = R.partition(case["cam_centers"], case["obs_ptr"], case["obs_point_id"], case["point_id"], case["point_xyz"],
                      case["point_error"], case["depth_centers"], C.grid_of(case), 100.0, max_n_cams=6,
                      rng=random.Random(1234))
    assert len(ref["chunks"]) > 0 and any(d[0] == "randint" for d in ref["draws"])
    _assert_equal(part, ref, "auto on the device")


def test_two_runs_are_bitwise_equal():
    case = C.cases()["3x3_333"]
    a, b = _run(case, (2, 7, True)), _run(case, (2, 7, True))
    for k in ("cell32", "cell64", "n_pts", "total", "blend", "cam_cell", "depth_cell"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(a.candidates, b.candidates) and len(a.chunks) == len(b.chunks) > 0
    for x, y in zip(a.chunks, b.chunks):
        assert np.array_equal(x.cameras, y.cameras) and np.array_equal(x.obs_offsets, y.obs_offsets)
        assert torch.equal(x.obs_index, y.obs_index) and torch.equal(x.points, y.points)


def test_duplicate_ids_raise():
    case = dict(C.cases()["3x3"])
    ids = case["point_id"].copy()
    ids[7] = ids[150]
    case["point_id"] = ids
    with pytest.raises(RuntimeError, match="same id"):
        _run(case, (5, 1500, True))


def test_bad_ids_raise():
    case = dict(C.cases()["3x3"])
    for bad in (-1, 2 ** 31 - 1):
        ids = case["point_id"].copy()
        ids[3] = bad
        with pytest.raises(ValueError, match="point_id"):
            _run(dict(case, point_id=ids), (5, 1500, True))


def test_oversized_camera_cell_product_raises():
    case = dict(C.cases()["empty_O"])
    M = len(case["cam_centers"])
    n = (2 ** 31 + M - 1) // M  # cells with M cells >= 2^31
    bbox = np.array([[-1e9, -1e9, -1e12], [1e9, 1e9, 1e12]], dtype=np.float32)
    case["grid"] = (bbox, n, 1)
    case["chunk_size"] = 0.5
    with pytest.raises(ValueError, match="2\\^31"):
        _run(case, (5, 1500, True))


def test_a_chunks_center_and_extent_crop_its_lidar_cloud():
    from gs_train.lidar import crop_bounds, prepare_chunk_cloud
    case = C.cases()["3x3"]
    part = _run(case, (5, 1500, True))
    chunk = part.chunks[-1]
    assert (chunk.i, chunk.j) == (1, 0)
    rng = np.random.default_rng(3)
    b = crop_bounds(chunk.center, chunk.extent)
    assert b.dtype == np.float32 and b[0] < b[1] and b[2] < b[3]
    # a cloud over the chunk and its neighbours, with points on the fp32 bounds and one step either side
    pts = rng.uniform([b[0] - 60, b[2] - 60, -3], [b[1] + 60, b[3] + 60, 20], (4000, 3)).astype(np.float32)
    k = 0
    for axis, vals in ((0, b[:2]), (1, b[2:])):
        for v in vals:
            for w in (np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))):
                pts[k, axis] = w
                pts[k, 1 - axis] = (b[2] + b[3]) / 2 if axis == 0 else (b[0] + b[1]) / 2
                k += 1
    cloud = prepare_chunk_cloud(torch.from_numpy(pts).to(DEV), None, chunk.center, chunk.extent, mesh=None,
                                lidar_init=False)
    want = (b[0] < pts[:, 0]) & (pts[:, 0] < b[1]) & (b[2] < pts[:, 1]) & (pts[:, 1] < b[3])
    assert 0 < want.sum() < len(pts)
    assert np.array_equal(_np(cloud.points), pts[want])


def test_the_library_rejects_bad_sizes_and_takes_empty_ones():
    import ctypes
    from diff_gaussian_rasterization._lib import ChunkGrid, last_error
    from gs_train._native import lib, ptr
    L = lib()
    INVALID = -1  # GSR_ERR_INVALID_ARGUMENT
    g = ctypes.byref(ChunkGrid(0.0, 0.0, 100.0, 3, 3))
    # M cells >= 2^31, an id table past 2^31 - 1 entries, grids without cells or outside +-1e12: no pointer is read
    assert L.gsr_chunk_camera_counts(2 ** 20, None, 0, None, 0, None, None, None, 2 ** 11, None, None, None, None) == INVALID
    assert "2^31" in last_error()
    assert L.gsr_chunk_camera_counts(2 ** 20, None, 0, None, 0, None, None, None, 2 ** 11 - 1, None, None, None, None) == INVALID
    assert "NULL" in last_error()  # the sizes pass: 2^20 (2^11 - 1) < 2^31
    assert L.gsr_chunk_id_table(1, None, 2 ** 31, None, None) == INVALID
    for bad in (ChunkGrid(0.0, 0.0, 100.0, 0, 3), ChunkGrid(0.0, 0.0, 0.0, 3, 3), ChunkGrid(-2e12, 0.0, 100.0, 3, 3),
                ChunkGrid(0.0, 0.0, 1e11, 3, 11), ChunkGrid(float("nan"), 0.0, 100.0, 3, 3),
                ChunkGrid(0.0, 0.0, 1.0, 2 ** 16, 2 ** 15)):
        assert L.gsr_chunk_classify_points(0, None, None, ctypes.byref(bad), None, None, None) == INVALID
        assert L.gsr_chunk_classify_centers(0, None, 0, None, ctypes.byref(bad), None, None, None) == INVALID
    # empty inputs: nothing to launch, no pointer needed
    assert L.gsr_chunk_classify_points(0, None, None, g, None, None, None) == 0
    assert L.gsr_chunk_classify_centers(0, None, 0, None, g, None, None, None) == 0
    mm = (ctypes.c_int64 * 2)(5, 5)
    assert L.gsr_chunk_id_range(0, None, mm, None) == 0 and list(mm) == [0, -1]
    assert L.gsr_chunk_id_table(0, None, 0, None, None) == 0
    assert L.gsr_chunk_camera_counts(0, None, 0, None, 0, None, None, None, 9, None, None, None, None) == 0
    # duplicate and out-of-range ids, on the device
    ids = torch.tensor([4, 2, 7, 2], dtype=torch.int64, device=DEV)
    table = torch.empty(8, dtype=torch.int32, device=DEV)
    assert L.gsr_chunk_id_table(4, ptr(ids), 8, ptr(table), None) == INVALID and "same id" in last_error()
    assert L.gsr_chunk_id_table(4, ptr(ids), 7, ptr(table), None) == INVALID and "not below T" in last_error()
    ids[3] = 0
    assert L.gsr_chunk_id_table(4, ptr(ids), 8, ptr(table), None) == 0
    assert table.tolist() == [3, -1, 1, -1, 0, -1, -1, 2]
    assert L.gsr_chunk_id_range(4, ptr(ids), mm, None) == 0 and list(mm) == [0, 7]
