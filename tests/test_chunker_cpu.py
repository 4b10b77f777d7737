"""CPU tests of the scene partition's host side (gs_train.chunker) and of the yardstick the GPU tests use:
tests/chunker_ref.py against hand-worked scenes, chunk_grid and fill_temporal_gaps on typed values, the
cases of tests/chunker_cases.py held to what makes them worth running, and the argument checks that need
no GPU."""
from __future__ import annotations

import random

import numpy as np
import pytest

import chunker_cases as C
import chunker_ref as R

F32 = np.float32


def _scene(cams, obs, points, depth=None):
    """cams: centres; obs: per camera the observed ids; points: (id, xyz, error) rows."""
    ptr = np.concatenate([[0], np.cumsum([len(o) for o in obs])]).astype(np.int64)
    flat = np.array([q for o in obs for q in o], dtype=np.int64)
    return dict(cam_centers=np.array(cams, dtype=F32).reshape(-1, 3), obs_ptr=ptr, obs_point_id=flat,
                point_id=np.array([p[0] for p in points], dtype=np.int64),
                point_xyz=np.array([p[1] for p in points], dtype=np.float64).reshape(-1, 3),
                point_error=np.array([p[2] for p in points], dtype=F32), depth_centers=depth)


def _ref(s, grid, cs, **kw):
    return R.partition(s["cam_centers"], s["obs_ptr"], s["obs_point_id"], s["point_id"], s["point_xyz"],
                       s["point_error"], s["depth_centers"], grid, cs, **kw)


# A 2 x 1 grid of 10 m cells from the origin: cell 0 is x < 10 (extended down), cell 1 is x > 10.
GRID2 = (np.array([[0, 0, -1e12], [20, 10, 1e12]], dtype=F32), 2, 1)


def test_reference_on_a_hand_worked_scene():
    points = [(5, (1.0, 1.0, 0.0), 1.0),      # row 0: cell 0
              (2, (10.0, 5.0, 0.0), 1.0),     # row 1: on the bound between the cells: neither
              (9, (12.0, 5.0, 3.0), 9.5),     # row 2: cell 1
              (7, (-50.0, -3.0, 0.0), 2.0),   # row 3: outside the grid on both axes: cell 0, extended
              (4, (15.0, 99.0, 0.0), 10.0),   # row 4: error 10: not in C; by fp64 position in cell 1
              (0, (0.0, 0.0, 0.0), 1.0),      # row 5: the origin point: cell 0 is x > -1e12: in C, never visible
              (11, (3.0, 3.0, 1e12), 1.0)]    # row 6: z on the bound: in no cell by fp64; float32(1e12) < 1e12: cell 0
    cams = [(5.0, 5.0, 0.0),                  # 0: IN cell 0
            (15.0, 5.0, 0.0),                 # 1: IN cell 1; centre inside ebox(0) = (-5, 15)
            (10.0, 5.0, 0.0),                 # 2: on the shared face: IN neither
            (5.0, 5.0, 1e12)]                 # 3: float32(1e12) < 1e12: IN cell 0
    obs = [[5, 5, 7, -1, 2, 0, 4, 11, 9], [9, 4, 6], [], [0]]
    s = _scene(cams, obs, points, depth=np.array([[5, 5, 0], [10, 5, 0], [19, 9.5, 0], [5, 5, 1e12]], dtype=np.float64))
    r = _ref(s, GRID2, 10.0, min_n_cams=0)
    assert r["cell32"].tolist() == [0, -1, 1, 0, R.NOT_IN_C, 0, 0]
    assert r["cell64"].tolist() == [0, -1, 1, 0, 1, 0, -1]
    # camera 0 sees 5, 5, 7, 11 (cell 0), 2 (no cell), 9 (cell 1); 0 is the origin, 4 is not in C
    assert r["total"].tolist() == [6, 1, 0, 0]
    assert r["n_pts"].tolist() == [[4, 1], [0, 1], [0, 0], [0, 0]]
    assert r["blend"].tolist() == [[5, 1], [0, 1], [0, 0], [1, 0]]  # the origin counts for np.isin
    assert r["candidates"].tolist() == [[0, 0, R.IN, 4, 6], [0, 3, R.IN, 0, 0], [1, 1, R.IN, 1, 1]]
    assert [(c["i"], c["j"]) for c in r["chunks"]] == [(0, 0), (1, 0)] and r["excluded"] == [] and r["draws"] == []
    a, b = r["chunks"]
    assert a["cameras"].tolist() == [0, 3] and b["cameras"].tolist() == [1]
    # kept observations, as indices into obs_point_id: ids 5, 5, 7, 0 of camera 0 (11 is out by its fp64 z); id 0
    # of camera 3
    assert [k.tolist() for k in a["obs"]] == [[0, 1, 2, 5], [12]]
    assert [k.tolist() for k in b["obs"]] == [[9, 10]]  # ids 9 and 4: the filter keeps a point outside C
    assert a["points"].tolist() == [0, 3, 5, 6] and b["points"].tolist() == [2]
    assert a["blend"].tolist() == [5, 1] and b["blend"].tolist() == [1]
    assert a["depth_cameras"].tolist() == [0] and b["depth_cameras"].tolist() == [2]
    assert a["center"].tolist() == [5.0, 5.0, 0.0] and a["extent"].tolist() == [10.0, 10.0, 2e12]
    assert b["center"].tolist() == [15.0, 5.0, 0.0]
    assert r["memberships32"].max() == 1 and r["memberships64"].max() == 1


class _Script:
    """A generator that returns what the test typed, and records what it was asked."""

    def __init__(self, values):
        self.values, self.asked = list(values), []

    def uniform(self, a, b):
        self.asked.append(("uniform", a, b))
        return self.values.pop(0)

    def randint(self, a, b):
        self.asked.append(("randint", a, b))
        return self.values.pop(0)


def _two_chunk_scene():
    """Cell 0 holds points 0..29, cell 1 points 100..129.  Cameras 0..2 sit in cell 0, camera 3 in cell 1;
    cameras 4 and 5 are far from both (outside either ebox) and see 12 / 15 points of cell 0 and 25 / 11 of
    cell 1; camera 6 is within ebox(1) only and sees 20 points of cell 1 (a near camera below 21: a draw)."""
    points = [(k, (1.0 + 0.25 * k, 2.0, 0.0), 1.0) for k in range(30)]
    points += [(100 + k, (11.0 + 0.25 * k, 2.0, 0.0), 1.0) for k in range(30)]
    cams = [(2, 2, 0), (3, 2, 0), (4, 2, 0), (12, 2, 0), (40, 2, 0), (-30, 2, 0), (22, 2, 0)]
    obs = [[0], [1], [2], [100],
           list(range(12)) + list(range(100, 125)),        # 4: 12 of 37, 25 of 37
           list(range(15)) + list(range(100, 111)) + [7] * 4,  # 5: 19 of 30 (duplicates count), 11 of 30
           list(range(100, 120))]                          # 6: 20 of 20
    return _scene(cams, obs, points)


def test_reference_interleaves_the_far_camera_draws_and_the_removals():
    s = _two_chunk_scene()
    # cell 0: cameras 4 (12/37 = 0.324) and 5 (19/30 = 0.633) draw; then 5 valid > 4: one removal.
    # cell 1: cameras 4 (25/37 = 0.676), 5 (11/30 = 0.367) and 6 (20/20) draw; 3 valid: no removal.
    rng = _Script([0.30, 0.49,   # cell 0: 0.30 < 0.324 valid; 0.49 < 0.633 valid -> valid 0 1 2 4 5
                   3,            # remove the valid camera number 3: camera 4 -> 0 1 2 5
                   0.45, 0.40, 0.2,  # cell 1: camera 4 valid, camera 5 (0.40 >= 0.367) not, camera 6 valid -> 3 4 6
                   ])
    r = _ref(s, GRID2, 10.0, min_n_cams=2, max_n_cams=4, rng=rng)
    assert rng.asked == [("uniform", 0, 0.5), ("uniform", 0, 0.5), ("randint", 0, 4), ("uniform", 0, 0.5),
                         ("uniform", 0, 0.5), ("uniform", 0, 0.5)]
    assert r["candidates"].tolist() == [[0, 0, 1, 1, 1], [0, 1, 1, 1, 1], [0, 2, 1, 1, 1], [0, 4, 3, 12, 37],
                                        [0, 5, 3, 19, 30], [1, 3, 1, 1, 1], [1, 4, 3, 25, 37], [1, 5, 3, 11, 30],
                                        [1, 6, 3, 20, 20]]
    assert [c["cameras"].tolist() for c in r["chunks"]] == [[0, 1, 2, 5], [3, 4, 6]]
    assert r["draws"] == [("uniform", 0, 4, 0.30), ("uniform", 0, 5, 0.49), ("randint", 0, 4, 3),
                          ("uniform", 1, 4, 0.45), ("uniform", 1, 5, 0.40), ("uniform", 1, 6, 0.2)]
    # with one observation more camera 6 is near (21 > 20) and does not draw; the removals follow each cell's draws
    s2 = _two_chunk_scene()
    s2["obs_point_id"] = np.concatenate([s2["obs_point_id"], [120]])
    s2["obs_ptr"][-1] += 1
    rng = _Script([0.4, 0.1,  # cell 0: camera 4 (0.4 >= 0.324) not valid, camera 5 valid -> 0 1 2 5
                   3,         # remove number 3: camera 5 -> 0 1 2
                   0.1, 0.3,  # cell 1: cameras 4 and 5 valid, camera 6 near -> 3 4 5 6
                   0])        # remove number 0: camera 3 -> 4 5 6
    r = _ref(s2, GRID2, 10.0, min_n_cams=2, max_n_cams=3, rng=rng)
    assert rng.asked == [("uniform", 0, 0.5), ("uniform", 0, 0.5), ("randint", 0, 3), ("uniform", 0, 0.5),
                         ("uniform", 0, 0.5), ("randint", 0, 3)]
    assert r["candidates"].tolist()[-1] == [1, 6, R.NEAR, 21, 21]
    assert [c["cameras"].tolist() for c in r["chunks"]] == [[0, 1, 2], [4, 5, 6]]


def test_reference_removal_indexes_the_valid_cameras_in_ascending_order():
    s = _two_chunk_scene()
    rng = _Script([0.0, 0.0, 0, 0, 0.0, 0.0, 0.0, 2])
    r = _ref(s, GRID2, 10.0, min_n_cams=0, max_n_cams=3, rng=rng)
    # cell 0: all five valid, removals 0 then 0: cameras 0 and 1 go.  cell 1: 3 4 5 6 valid, removal 2: camera 5
    assert rng.asked == [("uniform", 0, 0.5)] * 2 + [("randint", 0, 4), ("randint", 0, 3)] + [("uniform", 0, 0.5)] * 3 + \
        [("randint", 0, 3)]
    assert [c["cameras"].tolist() for c in r["chunks"]] == [[2, 4, 5], [3, 4, 6]]
    # min_n_cams equal to the count excludes; the draws are made all the same
    rng = _Script([0.0, 0.0, 0, 0, 0.0, 0.0, 0.0, 2])
    r = _ref(s, GRID2, 10.0, min_n_cams=3, max_n_cams=3, rng=rng)
    assert r["chunks"] == [] and r["excluded"] == [(0, 0), (1, 0)] and len(rng.asked) == 8
    # no far cameras: no draws at all
    rng = _Script([])
    r = _ref(s, GRID2, 10.0, min_n_cams=0, add_far_cams=False, rng=rng)
    assert rng.asked == [] and [c["cameras"].tolist() for c in r["chunks"]] == [[0, 1, 2], [3]]


def test_resolve_candidates_agrees_with_the_reference_on_every_case():
    from gs_train.chunker import resolve_candidates
    for name, run in C.all_runs():
        ref = C.reference(name, run)
        g = C.grid_of(C.cases()[name])
        got = resolve_candidates(ref["candidates"], g[1] * g[2], run[0], run[1], random.Random(0))
        emitted = [divmod(c, g[2]) for c in range(g[1] * g[2]) if got[c][1]]
        assert emitted == [(c["i"], c["j"]) for c in ref["chunks"]], (name, run)
        for c in ref["chunks"]:
            assert np.array_equal(got[c["cell"]][0], c["cameras"]), (name, run, c["cell"])
    # and asks the generator for the same things in the same order
    s = _two_chunk_scene()
    cand = _ref(s, GRID2, 10.0)["candidates"]
    rng = _Script([0.0, 0.0, 0, 0, 0.0, 0.0, 0.0, 2])
    got = resolve_candidates(cand, 2, 0, 3, rng)
    assert [g[0].tolist() for g in got] == [[2, 4, 5], [3, 4, 6]] and len(rng.asked) == 8


def test_chunk_grid_on_typed_values():
    from gs_train.chunker import chunk_grid
    cam = np.array([[0.0, 0.0, 1.0], [250.0, 130.0, 2.0], [100.0, 50.0, -4.0]], dtype=F32)
    bbox, n_w, n_h = chunk_grid(cam, 100.0, 0.2)
    # x: -20 .. 270, extent 290, padd 10: -25 .. 275.  y: -20 .. 150, extent 170, padd 30: -35 .. 165
    assert bbox.dtype == F32 and (n_w, n_h) == (3, 2)
    assert bbox.tolist() == [[-25.0, -35.0, F32(-1e12)], [275.0, 165.0, F32(1e12)]]
    # an extent that is already a whole number of chunks is padded by a whole chunk
    bbox, n_w, n_h = chunk_grid(np.array([[0, 0, 0], [160, 60, 0]], dtype=F32), 100.0, 0.2)
    assert (n_w, n_h) == (3, 2) and bbox[0].tolist()[:2] == [-70.0, -70.0] and bbox[1].tolist()[:2] == [230.0, 130.0]
    # float32 arithmetic, the % included: the steps typed out in float32
    cam = np.array([[0.1, 0.2, 0.0], [123.456, 77.7, 0.0]], dtype=F32)
    cs, pad = F32(33.3), F32(0.2 * 33.3)
    lo, hi = cam[0, :2] - pad, cam[1, :2] + pad
    ext = hi - lo
    assert ext.dtype == F32
    padd = np.array([cs - np.fmod(ext[0], cs), cs - np.fmod(ext[1], cs)], dtype=F32)
    lo, hi = lo - padd / F32(2), hi + padd / F32(2)
    bbox, n_w, n_h = chunk_grid(cam, 33.3, 0.2)
    assert np.array_equal(bbox[0, :2], lo) and np.array_equal(bbox[1, :2], hi)
    assert (n_w, n_h) == (5, 3)
    # the same steps in float64 give another x0: the float32 matters
    ext64 = (cam[1, :2].astype(np.float64) + 0.2 * 33.3) - (cam[0, :2].astype(np.float64) - 0.2 * 33.3)
    lo64 = cam[0, :2] - 0.2 * 33.3 - (33.3 - ext64 % 33.3) / 2
    assert not np.array_equal(lo64, bbox[0, :2].astype(np.float64))
    with pytest.raises(ValueError):
        chunk_grid(np.zeros((0, 3), F32))
    with pytest.raises(ValueError):
        chunk_grid(np.array([[0, np.nan, 0]], F32))
    with pytest.raises(ValueError):
        chunk_grid(cam, 0.0)


def test_camera_centers():
    from gs_train.chunker import camera_centers, qvec2rotmat
    # a quarter turn about z: R maps x to y; the centre is -R^T t
    q = np.array([np.sqrt(0.5), 0, 0, np.sqrt(0.5)])
    assert np.allclose(qvec2rotmat(q), [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    c = camera_centers([q, [1, 0, 0, 0]], [[1, 2, 3], [4, 5, 6]], np.float64)
    assert c.dtype == np.float64 and np.allclose(c, [[-2, 1, -3], [-4, -5, -6]], atol=1e-15)
    rng = np.random.default_rng(0)
    q = rng.normal(size=(5, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.normal(size=(5, 3)) * 100
    c32 = camera_centers(q, t)
    assert c32.dtype == F32
    for k in range(5):
        assert np.array_equal(c32[k], -qvec2rotmat(q[k]).astype(F32).T @ t[k].astype(F32))
    assert np.allclose(c32, camera_centers(q, t, np.float64), rtol=1e-5, atol=1e-4)


def test_fill_temporal_gaps_on_typed_sequences():
    from gs_train.chunker import fill_temporal_gaps
    n = 12
    order = list(range(n))
    xy = np.stack([np.arange(n) * 4.0, np.zeros(n)], 1)  # 4 m apart in time order
    assert fill_temporal_gaps([], order, xy) == set()
    # gaps inside: 3 and 6 selected -> 4 (after 3); 5 is the predecessor of the last: never examined.  Before
    # the first (2) and after the last (7)
    assert fill_temporal_gaps([3, 6], order, xy) == {4, 2, 7}
    # three selected: the middle one's predecessor and successor are examined
    assert fill_temporal_gaps([1, 5, 9], order, xy) == {0, 2, 4, 6, 10}  # not 8: the last one's predecessor
    # no gap: only before and after
    assert fill_temporal_gaps([4, 5, 6], order, xy) == {3, 7}
    # at the ends of the recording there is nothing before or after
    assert fill_temporal_gaps([0, 11], order, xy) == {1}
    assert fill_temporal_gaps([5], order, xy) == {4, 6}
    # the distance is strict and Euclidean
    far = xy.copy()
    far[4] = [far[3, 0] + 6.0, 8.0]  # exactly 10 from recording 3: not added
    assert fill_temporal_gaps([3, 6], order, far) == {2, 7}
    assert fill_temporal_gaps([3, 6], order, far, max_gap=10.5) == {4, 2, 7}
    # `order` is the time order: the same recordings under other row numbers
    perm = [7, 3, 9, 0, 5, 11, 2, 8, 1, 10, 4, 6]
    xyp = np.zeros((n, 2))
    xyp[perm] = xy
    assert fill_temporal_gaps([perm[3], perm[6]], perm, xyp) == {perm[4], perm[2], perm[7]}
    assert fill_temporal_gaps([perm[3], 99], perm, xyp) == {perm[2], perm[4]}  # 99 is not a recording


def test_cases_keep_every_point_in_at_most_one_cell():
    for name, run in C.all_runs():
        ref = C.reference(name, run)
        assert ref["memberships32"].max(initial=0) <= 1 and ref["memberships64"].max(initial=0) <= 1, name


def _cell_by_sum(x, x0, cs, n):
    """The cell on one axis when the upper bound is formed as bx(i) + cs (the wrong formula)."""
    for i in range(n):
        lo = -1e12 if i == 0 else x0 + i * cs
        hi = 1e12 if i == n - 1 else (x0 + i * cs) + cs
        if lo < x < hi:
            return i
    return -1


def test_cases_hold_what_they_are_for():
    cases = C.cases()
    separated = 0
    for name in ("1x4", "4x1", "3x3_333", "130x130"):
        c, ref = cases[name], C.reference(name, cases[name]["runs"][0])
        bbox, n_w, n_h = c["grid"]
        for r in np.nonzero(ref["cell64"] >= 0)[0]:
            i = _cell_by_sum(c["point_xyz"][r, 0], float(bbox[0, 0]), c["chunk_size"], n_w)
            j = _cell_by_sum(c["point_xyz"][r, 1], float(bbox[0, 1]), c["chunk_size"], n_h)
            separated += (i * n_h + j if i >= 0 and j >= 0 else -1) != ref["cell64"][r]
    assert separated > 0  # a point that bx(i) + cs as the upper bound puts elsewhere
    for name in ("1x1", "1x4", "4x1", "3x3", "3x3_333", "130x130"):
        c, ref = cases[name], C.reference(name, cases[name]["runs"][0])
        inC = ref["cell32"] != R.NOT_IN_C
        assert (ref["cell32"][inC] != ref["cell64"][inC]).any(), name
        assert (ref["cell64"] == -1).any() and (ref["cell32"] == -1).any()
        assert len(np.unique(c["point_id"])) == len(c["point_id"]) and (np.diff(c["point_id"]) < 0).any()
        L = c["point_id"][inC].max() + 1
        assert (c["point_id"][~inC] >= L).any() and (c["obs_point_id"] == -1).any()
        assert (~np.isin(c["obs_point_id"], c["point_id"]) & (c["obs_point_id"] >= 0)).any()
        states = set(ref["candidates"][:, 2].tolist())
        assert states == {R.IN, R.NEAR, R.DRAW}, (name, states)
    c, ref = cases["3x3"], C.reference("3x3", (5, 1500, True))
    counts = np.diff(c["obs_ptr"]).tolist()
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 5000):
        assert n in counts
    near = {(int(r[3]), int(r[2])) for r in ref["candidates"] if r[0] == 0}
    for want in ((11, R.DRAW), (20, R.DRAW), (21, R.NEAR), (21, R.DRAW), (25, R.IN), (25, R.NEAR), (25, R.DRAW)):
        assert want in near, want
    assert not (ref["candidates"][:, 3] == 10).any() or (ref["candidates"][ref["candidates"][:, 3] == 10, 2] == R.IN).all()
    assert (ref["n_pts"][:, 0] == 10).any()
    # centres exactly on a box face and on an ebox face (cs = 100: the bounds are float32 values)
    (lo, hi), _, (elo, ehi) = R.boxes(c["grid"][0], 100.0, 0, 0, 3, 3)
    x = c["cam_centers"][:, 0].astype(np.float64)
    assert (x == hi[0]).any() and (x == ehi[0]).any() and (x == elo[0]).any()
    # the host thresholds: a removal, an exclusion by min_n_cams == count, no far cameras
    runs = c["runs"]
    assert any(d[0] == "randint" for d in C.reference("3x3", runs[1])["draws"])
    first = ref["chunks"][0]
    assert runs[2][0] == len(first["cameras"]) and (first["i"], first["j"]) in C.reference("3x3", runs[2])["excluded"]
    assert C.reference("3x3", runs[3])["draws"] == [] and runs[3][2] is False
    # 64 consecutive observations in 64 cells; more cells than an LDS histogram holds
    c, ref = cases["130x130"], C.reference("130x130", (5, 1500, True))
    assert c["grid"][1] * c["grid"][2] == 16900 and len(c["cam_centers"]) == 8
    assert ((ref["n_pts"] > 0).sum(1) >= 64).any()
    for name in ("empty_N", "empty_M", "empty_O", "empty_D"):
        assert name in cases


def test_argument_checks_that_need_no_gpu():
    from gs_train.chunker import partition_scene
    c = C.cases()["3x3"]
    args = [c[k] for k in ("cam_centers", "obs_ptr", "obs_point_id", "point_id", "point_xyz", "point_error")]
    kw = dict(grid=c["grid"], device="cpu")

    def bad(i, value, **more):
        a = list(args)
        a[i] = value
        with pytest.raises(ValueError):
            partition_scene(*a, **{**kw, **more})

    bad(0, c["cam_centers"].astype(np.float64))
    bad(0, c["cam_centers"][:, :2])
    bad(1, c["obs_ptr"][:-1])
    bad(1, c["obs_ptr"][::-1].copy())
    bad(1, c["obs_ptr"] + 1)
    bad(1, c["obs_ptr"].astype(np.int32))
    bad(2, c["obs_point_id"].astype(np.int32))
    bad(3, c["point_id"][:-1])
    with np.errstate(over="ignore"):
        bad(4, c["point_xyz"].astype(np.float32))
    bad(5, c["point_error"].astype(np.float64))
    bad(0, c["cam_centers"], chunk_size=0.0)
    bad(0, c["cam_centers"], chunk_size=float("nan"))
    bad(0, c["cam_centers"], grid=(c["grid"][0], 0, 3))
    bad(0, c["cam_centers"], grid=(c["grid"][0], 2 ** 16, 2 ** 16))
    bad(0, c["cam_centers"], grid=(np.array([[-2e12, 0, 0], [0, 0, 0]], F32), 3, 3))
    bad(0, c["cam_centers"], depth_centers=np.zeros((4, 3), F32))
    bad(0, np.zeros((0, 3), F32), grid=None)
    M = len(c["cam_centers"])
    bad(0, c["cam_centers"], grid=(np.array([[-1e9, -1e9, 0], [0, 0, 0]], F32), (2 ** 31 + M - 1) // M, 1), chunk_size=0.5)
    with pytest.raises(RuntimeError, match="GPU"):  # valid arguments, no device: no fallback
        partition_scene(*args, **kw)
