"""The station render's host side (gs_train/station.py, include/gsr_station.h): camera grouping, the
exported symbols and ABI version, argument errors that need no device, and the synthetic layouts."""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np
import pytest

import station_cases as SC


def _f32(rows):
    return [np.asarray(r, np.float32) for r in rows]


def test_group_stations_bitwise_default():
    from gs_train.station import group_stations
    a, b = (1.0, 2.0, 3.0), (1.0, 2.0, np.nextafter(np.float32(3.0), np.float32(4.0)))
    centers = _f32([a, b, a, (0.0, 0.0, 0.0), b, a])
    assert group_stations(centers) == [[0, 2, 5], [1, 4], [3]]
    # -0.0 and 0.0 differ in their bits: the default groups bitwise-equal centres only
    assert group_stations(_f32([(0.0, 0.0, 0.0), (-0.0, 0.0, 0.0)])) == [[0], [1]]


def test_group_stations_decimals_is_the_reference_key():
    from gs_train.station import group_stations
    rng = np.random.default_rng(4)
    base = rng.uniform(-50, 50, (7, 3)).astype(np.float32)
    # six faces per station, centres jittered below and around the second decimal
    centers = [base[i % 7] + np.float32(rng.uniform(-0.004, 0.004)) for i in range(42)]
    centers += [base[0] + np.float32(0.02), base[1] - np.float32(0.011)]
    got = group_stations(centers, decimals=2)
    assert got == SC.reference_station_key(centers, 2)
    assert sorted(i for g in got for i in g) == list(range(len(centers)))
    assert len(got) > 7  # the jitter splits some stations at a rounding boundary, as it does in the reference


def test_group_stations_tol_single_and_order():
    from gs_train.station import group_stations
    c = _f32([(0, 0, 0), (10, 0, 0), (0.05, 0, 0), (10, 0.05, 0), (0.2, 0, 0), (0.09, 0, 0)])
    # distance to each group's FIRST member: 0.2 is outside 0.1 of (0,0,0) although 0.09 + ... chains would reach
    assert group_stations(c, tol=0.1) == [[0, 2, 5], [1, 3], [4]]
    assert group_stations(_f32([(1, 2, 3)])) == [[0]]
    assert group_stations(_f32([(1, 2, 3)]), tol=1.0) == [[0]]
    assert group_stations([]) == []
    # order preserved: groups by first appearance, members in camera order
    got = group_stations(_f32([(5, 5, 5), (1, 1, 1), (5, 5, 5), (1, 1, 1), (9, 9, 9)]))
    assert got == [[0, 2], [1, 3], [4]]
    with pytest.raises(ValueError):
        group_stations(c, tol=0.1, decimals=2)


def test_station_symbols_and_abi_version():
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    for name in ("gsr_rasterize_station_forward", "gsr_station_rows_scratch_bytes", "gsr_station_rows_layout",
                 "gsr_station_set_profiling", "gsr_station_stage_times_ms"):
        assert hasattr(L, name), name
        assert name in _lib.STATION_SIGNATURES
    assert L.gsr_abi_version() == 7 == _lib.ABI_VERSION
    assert _lib.STATION_MAX_FACES >= 6
    # scratch: 52 B of staged row + 1 B of flags per row at least; out-of-range F gives 0
    assert L.gsr_station_rows_scratch_bytes(1000, 6) >= 53 * 1000
    assert L.gsr_station_rows_scratch_bytes(1000, 0) == 0
    assert L.gsr_station_rows_scratch_bytes(1000, _lib.STATION_MAX_FACES + 1) == 0
    assert L.gsr_station_rows_scratch_bytes(0, 1) > 0
    # the rows buffer: 15 words per kept row, every array on a 256-byte boundary, faces in order
    kept = (ctypes.c_int64 * 3)(100, 0, 7)
    offs = (ctypes.c_size_t * 18)()
    total = L.gsr_station_rows_layout(3, kept, offs)
    o = list(offs)
    assert all(x % 256 == 0 for x in o) and o == sorted(o) and o[0] == 0
    assert o[1] - o[0] >= 1200 and o[2] - o[1] >= 2400 and total >= o[17] + 28 >= 60 * 107
    assert o[6:12] == [o[6]] * 6  # an empty face takes no room


def _call(F, views=1, projs=1, M=16, D=3, campos=1):
    """gsr_rasterize_station_forward with R = 0 and fake (never dereferenced) non-NULL pointers where
    `1` is given: every check below fails before any device work."""
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    cb = _lib.RESIZE_FN(lambda ctx, n: 0)
    K = (ctypes.c_int64 * 16)()
    p = lambda x: ctypes.c_void_p(4096) if x else None
    rc = L.gsr_rasterize_station_forward(cb, cb, cb, cb, None, None, 0, 0, D, M, None, None, None, None, None, None,
                                         None, None, 0, F, p(views), p(projs), p(campos), 1.0, 1.0, 64, 64, p(1), p(1),
                                         None, None, K, None, 0, None)
    return rc, _lib.last_error()


def test_station_argument_errors_without_a_device():
    from diff_gaussian_rasterization import _lib
    INVALID = -1  # GSR_ERR_INVALID_ARGUMENT
    rc, msg = _call(0)
    assert rc == INVALID and "F must be >= 1" in msg
    rc, msg = _call(-3)
    assert rc == INVALID and "F must be >= 1" in msg
    rc, msg = _call(_lib.STATION_MAX_FACES + 1)
    assert rc == INVALID and "GSR_STATION_MAX_FACES" in msg and str(_lib.STATION_MAX_FACES) in msg
    rc, msg = _call(4, views=0)
    assert rc == INVALID and "viewmatrices" in msg
    rc, msg = _call(4, projs=0)
    assert rc == INVALID and "projmatrices" in msg
    rc, msg = _call(4, campos=0)
    assert rc == INVALID and "cam_pos" in msg
    rc, msg = _call(4, M=9)
    assert rc == INVALID and "M = 16" in msg
    rc, msg = _call(4, D=4)
    assert rc == INVALID and "degree" in msg


def test_shell_layout_fills_every_octant():
    import torch
    h = SC.shell("cpu", skybox=400, leaves=4000)
    S, N = 400, h["means3D"].shape[0]
    leaves = h["means3D"][N - S - 4000:N - S]
    r = leaves.norm(dim=1)
    assert float(r.min()) >= 1.0 - 1e-4 and float(r.max()) <= 25.0 + 1e-3
    for rows in (leaves, h["means3D"][N - S:]):
        octant = ((rows[:, 0] > 0).long() * 4 + (rows[:, 1] > 0).long() * 2 + (rows[:, 2] > 0).long())
        counts = torch.bincount(octant, minlength=8)
        assert int(counts.min()) >= rows.shape[0] // 16, counts.tolist()  # 1/8 each, give or take
    with pytest.raises(ValueError):
        from gs_train.synthetic import synthetic_lod_hierarchy
        synthetic_lod_hierarchy(100, 64, 64, "cpu", layout="ring")


def test_frustum_layout_unchanged_from_parent_commit():
    """The default layout is bit for bit what it was before `layout` existed: the checksum below was
    taken from the parent commit's synthetic_lod_hierarchy(3000, 640, 360, "cpu", seed=5, skybox=40)
    over the nodes, the leaves' means and opacities (in Morton order) and the camera.  Those are the
    values made of exact operations on the generator's uniform stream (the opacities are drawn after
    the scales' and rotations' normal draws, so they also pin the stream's position after the line
    that now branches); exp / log of the normal draws go through the host's vector maths library and
    are compared with the explicit layout="frustum" call instead."""
    import torch
    from gs_train.synthetic import synthetic_lod_hierarchy
    h = synthetic_lod_hierarchy(3000, 640, 360, "cpu", seed=5, skybox=40)
    L, N = 3000, h["means3D"].shape[0] - 40
    s = hashlib.sha256()
    s.update(h["nodes"].numpy().tobytes())
    s.update(h["means3D"][N - L:N].numpy().tobytes())
    s.update(h["opacities"][N - L:N].numpy().tobytes())
    for k in ("view", "proj", "campos"):
        s.update(np.ascontiguousarray(h[k]).tobytes())
    assert s.hexdigest() == "530897001c3233c71794837edb6ea3907613b6f4c6a859ffd2aad52f5b8f66ee"
    g = synthetic_lod_hierarchy(3000, 640, 360, "cpu", seed=5, skybox=40, layout="frustum")
    for k in ("means3D", "scales", "rotations", "opacities", "shs", "nodes", "boxes"):
        assert torch.equal(h[k], g[k]), k


def test_cube_face_cameras():
    from gs_train.synthetic import cube_face_cameras
    c = (1.5, -0.25, 3.0)
    for n in (4, 6):
        cams = cube_face_cameras(128, n, c)
        assert len(cams) == n
        axes = []
        for cam in cams:
            assert cam["tanfovx"] == 1.0 == cam["tanfovy"] and cam["W"] == cam["H"] == 128
            assert cam["campos"].dtype == np.float32 and cam["campos"].tobytes() == np.asarray(c, np.float32).tobytes()
            V = cam["view"].astype(np.float64)  # W2C^T
            R = V[:3, :3].T
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-6)
            assert np.allclose(R @ np.asarray(c) + V[3, :3], 0, atol=1e-5)  # the centre maps to the camera origin
            axes.append(np.round(R[2]).astype(int).tolist())  # the world direction the face looks along
        assert len({tuple(a) for a in axes}) == n
        assert all(a[1] == 0 for a in axes[:4])  # the four horizontal faces
    with pytest.raises(ValueError):
        cube_face_cameras(128, 5)
