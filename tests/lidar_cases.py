"""The inputs of the LiDAR preparation tests, built here: meshes and points for the crop and the mesh
filter (MESH_CASES), one exact tie (TIE_CASE) and clouds for the voxel mean (VOXEL_CASES).  Every mesh
case is small enough for all pairs in float64 (P <= 4099, F <= 5000).

Placement.  A point "at the threshold" sits at max_distance (1 -+ DELTA) from its closest feature,
DELTA = 1e-3 (1e-2 in the scene shifted by 2000 m, where casting a coordinate to fp32 alone moves it
by up to 6e-5 m): 1e-4 m on either side of 0.1 m, above the band tests/test_lidar_cpu.py measures for
the fp32 evaluation, so the float64 reference alone decides every point.  Randomly drawn points are
held to the same: a draw whose float64 distance is within GUARD of a queried distance is not used.
TIE_CASE is not in MESH_CASES: its points lie at exactly max_distance = 0.125 from a triangle with
power-of-two coordinates, every fp32 operation of the rule is exact on them, and it is there for the
`<=` of the threshold."""
from __future__ import annotations

import functools

import numpy as np

MAX_DISTANCE = 0.1
QUERY_DISTANCES = (0.05, 0.1, 0.2)
TIE_DISTANCE = 0.125
DELTA = 1e-3
DELTA_SHIFTED = 1e-2
GUARD = 2e-4  # randomly drawn points closer than this to a queried distance are not used
POINT_COUNTS = (0, 1, 63, 64, 65, 257, 4099)
TRIANGLE_COUNTS = (1, 2, 4097)


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def feature_points(tri, md=MAX_DISTANCE, delta=DELTA):
    """Points whose closest feature of the non-degenerate triangle tri (3, 3) is the face interior,
    each edge and each vertex, at md (1 - delta) and md (1 + delta), and two at distance 0."""
    A, B, C = (np.asarray(v, np.float64) for v in tri)
    n = _unit(np.cross(B - A, C - A))
    G = (A + B + C) / 3
    out = []
    for f in (1 - delta, 1 + delta):
        d = md * f
        out += [G + n * d, G - n * d]  # the face, from both sides
        for P, Q, R in ((A, B, C), (B, C, A), (C, A, B)):
            e = _unit(Q - P)
            o = _unit((P + Q) / 2 - R - e * np.dot((P + Q) / 2 - R, e))  # in the plane, away from R
            M = P + (Q - P) * 0.37
            out += [M + o * d, M + _unit(o + n) * d, M + _unit(o - 0.5 * n) * d]  # the edge PQ
            out += [P + _unit(-_unit(Q - P) - _unit(R - P)) * d,  # the vertex P
                    P + _unit(-_unit(Q - P) - _unit(R - P) + 0.7 * n) * d]
    out += [A, 0.2 * A + 0.3 * B + 0.5 * C]  # distance 0: on a vertex, inside the face
    return np.array(out)


def _mesh(tris):
    """vertices, faces of independent triangles (F, 3, 3)."""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    return t.reshape(-1, 3).astype(np.float32), np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3)


def _case(vertices, faces, points, box=None):
    return {"vertices": np.ascontiguousarray(vertices, np.float32), "faces": np.ascontiguousarray(faces, np.int32),
            "points": np.ascontiguousarray(points, np.float32), "box": box}


def _terrain(nx, ny, pitch, rng, origin=(0.0, 0.0, 0.0)):
    """A height field of nx x ny quads (2 nx ny triangles), sides about `pitch`."""
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    z = 0.15 * np.sin(gx * 0.7) * np.cos(gy * 0.5) + rng.uniform(-0.03, 0.03, gx.shape)
    v = np.stack([gx * pitch, gy * pitch, z], -1).reshape(-1, 3) + np.asarray(origin)
    i = (gx[:-1, :-1] * (ny + 1) + gy[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([i, i + ny + 1, i + 1], 1), np.stack([i + 1, i + ny + 1, i + ny + 2], 1)])
    return v.astype(np.float32), f.astype(np.int32)


def _spread(vertices, n, rng, spread=0.35):
    v = np.asarray(vertices, np.float64)
    base = v[rng.integers(0, len(v), n)]
    return base + rng.uniform(-spread, spread, (n, 3)) * np.array([1.0, 1.0, 0.6])


def clear_of_thresholds(points, vertices, faces, n):
    """The first n of `points` (as fp32) whose float64 distance to the mesh is not within GUARD of a
    queried distance."""
    import lidar_ref
    p = np.asarray(points, np.float32)
    d = np.sqrt(lidar_ref.min_d2(p, vertices, faces))
    ok = np.ones(len(p), bool)
    for q in QUERY_DISTANCES + (TIE_DISTANCE,):
        ok &= ~(np.abs(d - q) < GUARD)
    rows = np.nonzero(ok)[0][:n]
    assert len(rows) == n
    return p[rows]


def _around(vertices, faces, n, rng, spread=0.35):
    """n points spread around the mesh's vertices (most within a few max_distance of the surface)."""
    return clear_of_thresholds(_spread(vertices, n + n // 8 + 8, rng, spread), vertices, faces, n)


TRI = np.array([[0.13, 0.21, 0.05], [0.52, 0.17, 0.11], [0.29, 0.55, -0.07]])


def _sizes(P, F, seed):
    rng = np.random.default_rng(seed)
    if F == 1:
        v, f = _mesh([TRI])
    elif F == 2:  # two triangles sharing an edge, folded
        v = np.array([TRI[0], TRI[1], TRI[2], [0.61, 0.58, 0.21]], np.float32)
        f = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    else:  # 64 x 32 quads and one more triangle standing on them
        v, f = _terrain(64, 32, 0.3, rng)
        v = np.concatenate([v, np.array([[3.0, 3.0, 0.5], [3.3, 3.1, 0.9], [3.1, 3.4, 1.2]], np.float32)])
        f = np.concatenate([f, np.array([[len(v) - 3, len(v) - 2, len(v) - 1]], np.int32)])
        assert len(f) == 4097
    return _case(v, f, _around(v, f, P, rng))


def _features(delta=DELTA, shift=0.0):
    """Closest-feature placement on a single triangle and on a folded pair; shift moves the scene."""
    t0 = (TRI + shift).astype(np.float32).astype(np.float64)
    t1 = (np.array([TRI[2], TRI[1], [0.61, 0.58, 0.21]]) + shift).astype(np.float32).astype(np.float64)
    far = np.array([[1.9, 1.8, 0.4], [2.3, 1.7, 0.5], [2.0, 2.2, 0.1]]) + shift  # its own neighbourhood
    far = far.astype(np.float32).astype(np.float64)
    v, f = _mesh([t0, t1, far])
    pts = np.concatenate([feature_points(t0, delta=delta), feature_points(t1, delta=delta),
                          feature_points(far, delta=delta)])
    return _case(v, f, pts)


def _neighbour_cells():
    """Small triangles (0.04 m) on a lattice whose pitch is no multiple of the cell: the points at
    max_distance (1 -+ DELTA) along the axes lie in cells the triangles' own boxes do not touch."""
    rng = np.random.default_rng(5)
    tris, pts = [], []
    for i in range(4):
        for j in range(4):
            for k in range(3):
                c = np.array([0.47 * i, 0.47 * j, 0.47 * k]) + rng.uniform(0, 0.05, 3)
                t = c + rng.uniform(-0.02, 0.02, (3, 3))
                t = t.astype(np.float32).astype(np.float64)
                tris.append(t)
                pts.append(feature_points(t))
    v, f = _mesh(tris)
    return _case(v, f, np.concatenate(pts))


def _oversize():
    """A 50 m triangle across the whole box (the oversize path) over a patch of small ones, points
    near its middle on both sides of the threshold, far from every small triangle."""
    rng = np.random.default_rng(6)
    v, f = _terrain(8, 8, 0.3, rng, origin=(20.0, 20.0, -3.0))
    big = np.array([[0.0, 0.0, 1.0], [50.0, 2.0, 2.5], [3.0, 50.0, 0.5]], np.float32).astype(np.float64)
    big2 = np.array([[50.0, 50.0, 4.0], [50.0, 2.0, 2.5], [3.0, 50.0, 0.5]], np.float32).astype(np.float64)
    f = np.concatenate([f, np.array([[len(v), len(v) + 1, len(v) + 2], [len(v) + 3, len(v) + 4, len(v) + 5]], np.int32)])
    v = np.concatenate([v, big.astype(np.float32), big2.astype(np.float32)])
    n = _unit(np.cross(big[1] - big[0], big[2] - big[0]))
    pts = [feature_points(big), feature_points(big2)]
    for a, b in rng.uniform(0.15, 0.4, (40, 2)):  # near the middle of the big triangle
        q = big[0] + a * (big[1] - big[0]) + b * (big[2] - big[0])
        pts.append(np.array([q + n * MAX_DISTANCE * (1 - DELTA), q - n * MAX_DISTANCE * (1 + DELTA), q]))
    pts.append(clear_of_thresholds(_spread(v[:81], 120, rng), v, f, 100))
    return _case(v, f, np.concatenate(pts))


def _degenerate():
    """Zero-area triangles: three collinear vertices, two coincident ones, three coincident ones --
    tested as the segment or the point they cover."""
    A, B = np.array([0.1, 0.2, 0.3]), np.array([0.6, 0.45, 0.2])
    seg3 = [A, (A + B) / 2, B]  # collinear in float64; in fp32 as good as: the area is rounding
    seg2 = [A + 2.0, A + 2.0, B + 2.0]
    seg2b = [A + 4.0, B + 4.0, B + 4.0]
    pt = [np.array([1.5, 1.5, 1.5])] * 3
    tris = [np.asarray(t, np.float32).astype(np.float64) for t in (seg3, seg2, seg2b, pt)]
    v, f = _mesh(tris)
    pts = []
    for t in tris[:3]:
        P, Q = t[0], t[2]
        e = _unit(Q - P)
        o = _unit(np.cross(e, [0.3, -0.2, 0.9]))
        for fct in (1 - DELTA, 1 + DELTA):
            d = MAX_DISTANCE * fct
            pts += [P + (Q - P) * 0.41 + o * d, P - e * d, Q + e * d, P + _unit(o - e) * d, P + (Q - P) * 0.5]
    for fct in (1 - DELTA, 1 + DELTA):
        for dirn in ([1, 0, 0], [0, -1, 0], [0.3, 0.4, -0.5]):
            pts.append(tris[3][0] + _unit(dirn) * MAX_DISTANCE * fct)
    pts.append(tris[3][0])
    return _case(v, f, np.array(pts))


def _needles():
    """Needles of aspect 1e4: 1 m long, 1e-4 m wide, in general position."""
    rng = np.random.default_rng(8)
    tris, pts = [], []
    for k in range(6):
        P = rng.uniform(0, 3, 3)
        e = _unit(rng.normal(size=3))
        w = _unit(np.cross(e, rng.normal(size=3)))
        t = np.array([P, P + e, P + 0.5 * e + 1e-4 * w]).astype(np.float32).astype(np.float64)
        tris.append(t)
        n = _unit(np.cross(t[1] - t[0], t[2] - t[0]))
        o = _unit(np.cross(n, t[1] - t[0]))
        o = o if np.dot(o, t[2] - t[0]) < 0 else -o  # in the plane, away from the third vertex
        for fct in (1 - DELTA, 1 + DELTA):
            d = MAX_DISTANCE * fct
            for s in (0.1, 0.5, 0.9):
                M = t[0] + (t[1] - t[0]) * s
                pts += [M + n * d, M - n * d, M + o * d, M + _unit(n + o) * d, M + _unit(o - n) * d]
            pts += [t[0] - _unit(t[1] - t[0]) * d, t[1] + _unit(t[1] - t[0]) * d]
        pts.append(t[0] + (t[1] - t[0]) * 0.3)
    v, f = _mesh(tris)
    return _case(v, f, np.array(pts))


def _fan():
    """5000 small triangles fanned around one apex: one cell's list holds them all (the wave's path)."""
    rng = np.random.default_rng(9)
    k = np.arange(5000)
    th = k * (2 * np.pi / 5000) * 7  # seven turns
    r = 0.03 + 0.02 * (k % 13) / 13
    z = 0.04 * np.sin(k * 0.01)
    rim = np.stack([r * np.cos(th), r * np.sin(th), z], 1)
    v = np.concatenate([[[0.0, 0.0, 0.0]], rim]).astype(np.float32)
    f = np.stack([np.zeros(5000, np.int64), 1 + k, 1 + (k + 1) % 5000], 1).astype(np.int32)
    pts = rng.uniform(-0.3, 0.3, (300, 3)) * np.array([1, 1, 0.7])
    return _case(v, f, clear_of_thresholds(pts, v, f, 257))


def _placement():
    """A terrain with a crop box: points far outside the mesh's box, in empty cells, exactly on the
    crop planes (dropped: the inequalities are strict), NaN and Inf points."""
    rng = np.random.default_rng(10)
    v, f = _terrain(20, 14, 0.3, rng)  # 6 m x 4.2 m
    center, extent = (3.0, 2.0, 0.0), (4.0, 2.0, 100.0)  # planes x = 1, 5 and y = 1, 3: exact in fp32
    pts = [_around(v, f, 600, rng)]
    pts.append(rng.uniform(-30, 30, (60, 3)))  # far outside the mesh's box
    pts.append(np.stack([rng.uniform(0, 6, 60), rng.uniform(0, 4.2, 60), rng.uniform(1.0, 4.0, 60)], 1))  # empty cells
    on = _spread(v, 80, rng, 0.05)
    on[:20, 0], on[20:40, 0], on[40:60, 1], on[60:80, 1] = 1.0, 5.0, 1.0, 3.0
    pts.append(on)
    beside = _spread(v, 40, rng, 0.05)  # one fp32 step inside the planes: kept by the crop
    beside[:20, 0] = np.nextafter(np.float32(1.0), np.float32(2.0))
    beside[20:, 1] = np.nextafter(np.float32(3.0), np.float32(2.0))
    pts.append(beside)
    bad = _spread(v, 12, rng, 0.05)
    bad[0, 0] = bad[1, 1] = bad[2, 2] = np.nan
    bad[3, 0] = bad[4, 1] = bad[5, 2] = np.inf
    bad[6, 0] = bad[7, 1] = bad[8, 2] = -np.inf
    bad[9] = np.nan
    pts.append(bad)
    return _case(v, f, np.concatenate(pts), box=(center, extent))


def _shifted():
    """The whole scene 2000 m from the origin: the feature placement and a terrain with random points."""
    rng = np.random.default_rng(11)
    a = _features(delta=DELTA_SHIFTED, shift=2000.0)
    v, f = _terrain(12, 12, 0.3, rng, origin=(2003.0, 2003.0, 2000.0))
    vv, ff = np.concatenate([a["vertices"], v]), np.concatenate([a["faces"], f + len(a["vertices"])])
    pts = clear_of_thresholds(_spread(v, 460, rng), vv, ff, 400)
    return _case(vv, ff, np.concatenate([a["points"], pts]),
                 box=((2002.0, 2002.0, 0.0), (8.0, 8.0, 1.0)))


def _builders():
    b = {}
    seed = 100
    for P, F in ((0, 1), (1, 1), (63, 1), (64, 2), (65, 2), (257, 2), (257, 4097), (4099, 4097), (4099, 1)):
        b[f"sizes_P{P}_F{F}"] = functools.partial(_sizes, P, F, seed)
        seed += 1
    b.update(features=_features, neighbour_cells=_neighbour_cells, oversize=_oversize, degenerate=_degenerate,
             needles=_needles, fan=_fan, placement=_placement, shifted=_shifted)
    return b


_BUILDERS = _builders()
MESH_CASES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def mesh_case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def mesh_case_d2(name):
    """The float64 all-pairs d2 of the case's points (computed once per process, never changed)."""
    import lidar_ref
    c = mesh_case(name)
    d2 = lidar_ref.min_d2(c["points"], c["vertices"], c["faces"], np.float64)
    d2.setflags(write=False)
    return d2


# ---- one cell, one run: the query walk's own boundaries -----------------------------------------

ONE_CELL_COUNTS = (16, 17, 64, 65)  # the lane's longest run, the wave's shortest, one slice, a slice and one
ONE_CELL_NEAR = 0.03                # the distance of a point near at every queried distance
_ONE_CELL_D = (ONE_CELL_NEAR, 0.5, 0.07, 0.15)  # by row % 4: near at every distance, at none, from 0.1, at 0.2


@functools.lru_cache(maxsize=None)
def one_cell_case(F):
    """F triangles of 1 cm inside a cube of 0.19 m, below the cell edge of an index built for
    MAX_DISTANCE (0.2 m): one cell, one run of F references in triangle order.  The first F - 1 sit in
    the cube's low corner and the last one in the opposite corner 0.31 m away, so it alone is in reach of
    the points, which lie beyond it on the diagonal: whoever finds a triangle has read the end of the
    run.  "points" is (3, 65, 3), a second wave of one lane each: [0] distances by row % 4 as
    _ONE_CELL_D (the 0.5 m ones have no vertex in reach on any axis and do not search); [1], [2] row 0 /
    row 63 alone at ONE_CELL_NEAR and every other row 10 m away, so the wave's broadcast has its owner
    at either end."""
    rng = np.random.default_rng(300 + F)
    c = np.concatenate([rng.uniform(0.0, 0.02, (F - 1, 1, 3)), np.full((1, 1, 3), 0.18)])
    v, f = _mesh(c + rng.uniform(0.0, 0.01, (F, 3, 3)))
    last = v[-3:].astype(np.float64)
    tip = last[np.argmax(last.sum(1))]  # the last triangle's vertex farthest along the diagonal
    u = _unit([1.0, 1.0, 1.0])
    side = rng.uniform(-0.002, 0.002, (65, 3))
    mixed = tip + u * np.array(_ONE_CELL_D)[np.arange(65) % 4, None] + side
    sets = [mixed]
    for lane in (0, 63):
        p = tip + 10.0 + side
        p[lane] = tip + u * ONE_CELL_NEAR + side[lane]
        sets.append(p)
    return _case(v, f, np.array(sets))


# max_distance = 0.125 and a triangle with n = (0, 0, 1): the points at height 0.125 have d2 = T exactly
TIE_CASE = _case(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32),
                 np.array([[0.25, 0.25, 0.125], [0.25, 0.5, -0.125], [-0.125, 0.5, 0.0], [1.125, 0.0, 0.0],
                           [0.25, 0.25, 0.1250001], [0.25, 0.25, 0.1249999]], np.float32))
TIE_EXPECTED = np.array([True, True, True, True, False, True])


# ---- the voxel mean's clouds ------------------------------------------------------------------

def _voxel_builders():
    def one_point():
        return np.array([[1.5, -2.25, 3.0]], np.float32), np.array([[0.2, 0.4, 0.6]], np.float32), 0.25

    def one_voxel():
        rng = np.random.default_rng(20)
        return rng.uniform(10.0, 10.2, (500, 3)).astype(np.float32), rng.uniform(0, 1, (500, 3)).astype(np.float32), 1.0

    def on_faces():
        # s = 0.25, lo = 0: the voxel faces lie at 0.125 + 0.25 k, exact in fp32 and in fp64; a point on
        # a face belongs to the upper voxel (floor)
        k = np.arange(0, 9)
        face = 0.125 + 0.25 * k
        g = np.array(np.meshgrid(face, face, face[:3], indexing="ij")).reshape(3, -1).T
        pts = np.concatenate([[[0.0, 0.0, 0.0]], g, g - [0.0, 2.0 ** -20, 0.0]])
        rng = np.random.default_rng(21)
        return pts.astype(np.float32), rng.uniform(0, 1, pts.shape).astype(np.float32), 0.25

    def run_lengths():
        # voxels with 1, 64, 65 and 3000 points (a lane's run, the wave's, with a ragged last slice)
        rng = np.random.default_rng(22)
        parts = [rng.uniform(0.0, 0.2, (n, 3)) + [2.0 * i, 0.5 * i, 0.0] for i, n in enumerate((1, 64, 65, 3000))]
        pts = np.concatenate(parts)
        perm = rng.permutation(len(pts))
        return pts[perm].astype(np.float32), rng.uniform(0, 1, pts.shape).astype(np.float32), 0.5

    def no_colors():
        rng = np.random.default_rng(23)
        return rng.uniform(-3, 3, (257, 3)).astype(np.float32), None, 0.7

    def street():
        rng = np.random.default_rng(24)
        pts = rng.uniform(0, 1, (4099, 3)) * [2.0, 1.5, 0.3] + [2000.0, -300.0, 12.0]
        return pts.astype(np.float32), rng.uniform(0, 1, (4099, 3)).astype(np.float32), (1.0 / 2000) ** (1 / 3)

    return dict(one_point=one_point, one_voxel=one_voxel, on_faces=on_faces, run_lengths=run_lengths,
                no_colors=no_colors, street=street)


_VOXEL_BUILDERS = _voxel_builders()
VOXEL_CASES = tuple(_VOXEL_BUILDERS)


@functools.lru_cache(maxsize=None)
def voxel_case(name):
    """(points, colors or None, voxel_size)"""
    return _VOXEL_BUILDERS[name]()


# a cloud 1000 m across at a voxel of 1e-7 m: 1e10 voxels along an axis
REJECTED_VOXEL = (np.array([[0.0, 0.0, 0.0], [1000.0, 1.0, 1.0]], np.float32), 1e-7)
