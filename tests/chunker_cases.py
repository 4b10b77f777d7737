"""Inputs of the scene-partition tests (test_chunker_cpu.py, test_gpu_chunker.py): the smallest scenes
at which each kernel of csrc/chunker.hip can go wrong.

A case is a dict: cam_centers, obs_ptr, obs_point_id, point_id, point_xyz, point_error, depth_centers,
grid ((bbox, n_w, n_h), or None: chunk_grid's own), chunk_size, and `runs`, the (min_n_cams, max_n_cams,
add_far_cams) triples it is run with.  reference(name, run) is the per-chunk rule on it, computed once."""
from __future__ import annotations

import functools

import numpy as np

import chunker_ref as R

X0 = np.float32(-200.1234)   # not short decimals; with cs = 100 every bx(i), by(j) here is also a float32
Y0 = np.float32(17.12345)
F32, F64 = np.float32, np.float64


def _bx(o, i, cs):
    return float(o) + float(i) * float(cs)


def _around(b):
    """fp64 values at and around a bound b: b, one fp64 step and one fp32 step either side.  The fp64
    neighbours round to the same float32 as b, which lies on one side of b unless b is a float32: those
    rows have cell32 != cell64."""
    f = F32(b)
    return [b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf), float(np.nextafter(f, F32(-np.inf))), float(f),
            float(np.nextafter(f, F32(np.inf)))]


class _Scene:
    def __init__(self, n_w, n_h, cs, seed):
        self.n_w, self.n_h, self.cs = n_w, n_h, float(cs)
        self.rng = np.random.default_rng(seed)
        self.bbox = np.array([[X0, Y0, -1e12], [F32(X0 + F32(n_w * cs)), F32(Y0 + F32(n_h * cs)), 1e12]], dtype=F32)
        self.xyz, self.err, self.known_cell = [], [], []   # known_cell: by construction, -1: not relied on
        self.cams, self.obs = [], []

    def mid(self, i, j):
        return np.array([(_bx(X0, i, self.cs) + _bx(X0, i + 1, self.cs)) / 2,
                         (_bx(Y0, j, self.cs) + _bx(Y0, j + 1, self.cs)) / 2, 0.0])

    def point(self, p, err=1.0, cell=-1):
        self.xyz.append(np.asarray(p, dtype=F64))
        self.err.append(F32(err))
        self.known_cell.append(cell)
        return len(self.xyz) - 1

    def interior(self, i, j, n, err=None):
        """n random points well inside cell (i, j); returns their rows."""
        rows = []
        for _ in range(n):
            p = self.mid(i, j) + np.append(self.rng.uniform(-0.4, 0.4, 2) * self.cs, self.rng.uniform(-5, 30))
            rows.append(self.point(p, self.rng.uniform(0, 5) if err is None else err, i * self.n_h + j))
        return rows

    def boundary_points(self, xs, ys):
        cs, n_w, n_h = self.cs, self.n_w, self.n_h
        for i in xs:
            vals = _around(_bx(X0, i, cs))
            if i < n_w:  # the upper bound is bx(i + 1), not bx(i) + cs: both values, whether they differ or not
                vals += [_bx(X0, i, cs) + cs, _bx(X0, i + 1, cs)]
            for k, v in enumerate(vals):
                self.point([v, self.mid(0, k % n_h)[1], 1.0])
        for j in ys:
            vals = _around(_bx(Y0, j, cs))
            if j < n_h:
                vals += [_bx(Y0, j, cs) + cs, _bx(Y0, j + 1, cs)]
            for k, v in enumerate(vals):
                self.point([self.mid(k % n_w, 0)[0], v, -2.0])
        # the outer edge is extended; z = +-1e12 is out, one step inside is in; NaN, Inf, beyond float32
        m = self.mid(0, 0)
        far_x, far_y = _bx(X0, n_w, cs), _bx(Y0, n_h, cs)
        for p in ([float(X0) - 50.0, m[1], 0], [far_x + 1000.0, m[1], 0], [m[0], float(Y0) - 1e6, 0],
                  [m[0], far_y + 77.0, 0], [-1e12, m[1], 0], [np.nextafter(-1e12, 0), m[1], 0], [1e12, m[1], 0],
                  [m[0], 1e12, 0], [m[0], np.nextafter(1e12, 0), 0], [m[0], m[1], 1e12], [m[0], m[1], -1e12],
                  [m[0], m[1], np.nextafter(1e12, 0)], [m[0], m[1], np.nextafter(-1e12, 0)], [np.nan, m[1], 0],
                  [m[0], np.nan, 0], [m[0], m[1], np.nan], [np.inf, m[1], 0], [-np.inf, m[1], 0], [m[0], np.inf, 0],
                  [m[0], m[1], -np.inf], [1e300, m[1], 0], [m[0], -1e300, 0]):
            self.point(p)

    def camera(self, center, obs_ids):
        self.cams.append(np.asarray(center, dtype=F32))
        self.obs.append(np.asarray(obs_ids, dtype=np.int64).reshape(-1))
        return len(self.cams) - 1


def _finish(s, ids, depth, grid=True, runs=((5, 1500, True),)):
    M = len(s.cams)
    obs_ptr = np.zeros(M + 1, np.int64)
    obs_ptr[1:] = np.cumsum([len(o) for o in s.obs])
    return dict(cam_centers=np.array(s.cams, dtype=F32).reshape(-1, 3), obs_ptr=obs_ptr,
                obs_point_id=np.concatenate(s.obs + [np.zeros(0, np.int64)]), point_id=np.asarray(ids, dtype=np.int64),
                point_xyz=np.array(s.xyz, dtype=F64).reshape(-1, 3), point_error=np.array(s.err, dtype=F32),
                depth_centers=depth, grid=(s.bbox, s.n_w, s.n_h) if grid else None, chunk_size=s.cs, runs=tuple(runs))


def _scene(n_w, n_h, cs, seed, big=False, full=True):
    """The shared construction; big: the 130 x 130 grid (few cameras, bounds at a few indices only)."""
    s = _Scene(n_w, n_h, cs, seed)
    rng = s.rng
    t = (0, 0)                                   # the target cell of the threshold cameras
    target = s.interior(*t, 40)
    other_cells = [(i, j) for i in range(min(n_w, 3)) for j in range(min(n_h, 3)) if (i, j) != t]
    others = [r for c in other_cells for r in s.interior(*c, 12)]
    others = np.array(others, dtype=np.int64)    # none in a 1 x 1 grid
    xs = range(n_w + 1) if not big else (0, 1, 64, 65, n_w - 1, n_w)
    ys = range(n_h + 1) if not big else (0, 1, 2, 127, n_h - 1, n_h)
    s.boundary_points(xs, ys)
    origin = s.point([0.0, 0.0, 0.0], 0.5)                             # a C point exactly at the origin
    e10 = s.point(s.mid(0, 0) + [1, 2, 3], 10.0)                       # error exactly 10: out
    e_below = s.point(s.mid(0, 0) + [2, 2, 3], np.nextafter(F32(10), F32(0)))  # the float32 just below: in
    e_nan = s.point(s.mid(0, 0) + [3, 2, 3], np.nan)
    bad = s.interior(0, 0, 6, err=50.0)                                # not in C
    N = len(s.xyz)
    ids = rng.choice(3 * N, N, replace=False).astype(np.int64)         # unsorted, with gaps
    top = int(np.argmax(ids))                                          # the largest id: give it to a row outside C,
    ids[top], ids[bad[0]] = ids[bad[0]], ids[top]                      # so that id >= L exists among the points
    missing = np.setdiff1d(np.arange(3 * N), ids)[:8]                  # ids with no point
    beyond = np.array([3 * N + 5, 2 ** 40])

    def noise(n):
        """n observation ids of every kind, duplicates included, none of them visible in the target cell."""
        pool = np.concatenate([ids[others], ids[bad], missing, beyond, [-1, -1, -1], [ids[origin], ids[e10], ids[e_nan]]])
        return rng.choice(pool, n, replace=True)

    def seen(n):
        """n distinct visible points of the target cell."""
        return ids[rng.choice(target, n, replace=False)]

    c0 = s.mid(*t)
    (lo, hi), _, (elo, ehi) = R.boxes(s.bbox, cs, 0, 0, n_w, n_h)
    near, far = c0 + [0.9 * cs, 0, 2], c0 + [1.6 * cs, 0, 2]       # outside box(t): inside / outside ebox(t)
    for n in (10, 11, 20, 21) if not big else ():
        s.camera(near, rng.permutation(np.concatenate([seen(n), noise(30)])))
        s.camera(far, rng.permutation(np.concatenate([seen(n), noise(3 * n)])))
    if big:  # eight cameras in all
        for centre, n in ((near, 21), (near, 20), (far, 11), (far, 10), (c0, 25), (c0 + [1, 1, 0], 12)):
            s.camera(centre, rng.permutation(np.concatenate([seen(n), noise(2 * n)])))
    # centres on (float32-nearest to) a box face and an ebox face of the target cell, and one step either side
    if not big:
        for b in (hi[0], ehi[0], elo[0]):
            f = F32(b)
            for v in (np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))):
                s.camera([v, c0[1], 1.0], np.concatenate([seen(25), noise(5)]))
        s.camera([c0[0], F32(ehi[1]), 1.0], np.concatenate([seen(25), noise(5)]))
        s.camera([c0[0], c0[1], F32(2e12)], np.concatenate([seen(25), noise(5)]))      # the float32 under ebox's z face
        s.camera([c0[0], c0[1], F32(1e12)], np.concatenate([seen(25), noise(5)]))      # the float32 under box's z face
        s.camera([c0[0], c0[1], np.nextafter(F32(1e12), F32(np.inf))], np.concatenate([seen(25), noise(5)]))
        s.camera([c0[0], c0[1], np.nextafter(F32(2e12), F32(np.inf))], np.concatenate([seen(25), noise(5)]))
    if full:
        every = np.concatenate([ids, missing, beyond, [-1]])
        for n in (0, 1, 63, 64, 65, 255, 256, 257):
            i, j = rng.integers(n_w), rng.integers(n_h)
            s.camera(s.mid(i, j) + [3, -4, 1.5], rng.choice(every, n, replace=True))
        s.camera(c0 + [1, 1, 1], rng.choice(np.concatenate([ids[target], [ids[origin]]]), 5000, replace=True))
        s.camera(c0 + [-2, 1, 1], np.concatenate([seen(3), seen(3)]))          # IN with few points
        for k in range(6):                                                       # plain cameras inside the target
            s.camera(c0 + [k, -k, 1], np.concatenate([seen(15), noise(10)]))
    # 64 consecutive observations in as many cells as the grid has, up to 64
    spread = [(k % n_w, (2 * k + k // n_w) % n_h) for k in range(64)]
    spread = list(dict.fromkeys(spread))
    if big:
        rows = [s.interior(i, j, 1)[0] for i, j in spread]
        new = np.setdiff1d(np.arange(3 * N), ids)[8:8 + len(rows)]       # unused ids below the largest
        ids = np.concatenate([ids, new])
        s.camera(s.mid(5, 5), np.concatenate([noise(7), new, noise(3)]))
        s.camera([F32(hi[0]), c0[1], 1.0], np.concatenate([seen(25), noise(5)]))
    else:
        per_cell = {}
        for r in target + list(others):
            per_cell.setdefault(s.known_cell[r], []).append(r)
        cyc = [ids[per_cell[c][k // len(per_cell) % len(per_cell[c])]] for k in range(64)
               for c in [sorted(per_cell)[k % len(per_cell)]]]
        s.camera(s.mid(n_w - 1, n_h - 1), np.concatenate([noise(7), cyc, noise(3)]))
    depth = np.array([s.mid(0, 0), s.mid(n_w - 1, n_h - 1) + [1, 1, 1], [float(X0), s.mid(0, 0)[1], 0],
                      [_bx(X0, 1, cs), s.mid(0, 0)[1], 0], [np.nextafter(_bx(X0, 1, cs), -np.inf), s.mid(0, 0)[1], 0],
                      [s.mid(0, 0)[0], s.mid(0, 0)[1], 1e12], [float(X0) - 5, 0, 0], [np.nan, 0, 0]], dtype=F64)
    return s, ids, depth


def _auto_case():
    """A scene whose grid is chunk_grid's own (3 x 3 at cs = 100): cameras and points around it."""
    rng = np.random.default_rng(77)
    cam = np.concatenate([[[3.3, -7.7, 1.0], [253.1, 241.9, 2.0]], rng.uniform([5, -5, 0], [250, 240, 3], (22, 3))]).astype(F32)
    from gs_train.chunker import chunk_grid
    bbox, n_w, n_h = chunk_grid(cam, 100.0, 0.2)
    assert (n_w, n_h) == (3, 3)
    xyz = rng.uniform([-60, -70, -3], [310, 300, 30], (400, 3))
    for i in range(4):  # points at and around this grid's own bounds
        for k, v in enumerate(_around(_bx(bbox[0, 0], i, 100.0))):
            xyz[6 * i + k, 0] = v
        for k, v in enumerate(_around(_bx(bbox[0, 1], i, 100.0))):
            xyz[24 + 6 * i + k, 1] = v
    err = rng.uniform(0, 12, 400).astype(F32)
    ids = rng.choice(1500, 400, replace=False).astype(np.int64)
    obs = [rng.choice(np.concatenate([ids, [-1, 1501, 7]]), n, replace=True) for n in rng.integers(0, 400, len(cam))]
    ptr = np.zeros(len(cam) + 1, np.int64)
    ptr[1:] = np.cumsum([len(o) for o in obs])
    depth = rng.uniform([-40, -40, 0], [300, 300, 3], (15, 3))
    return dict(cam_centers=cam, obs_ptr=ptr, obs_point_id=np.concatenate(obs).astype(np.int64), point_id=ids,
                point_xyz=xyz, point_error=err, depth_centers=depth, grid=None, chunk_size=100.0,
                runs=((5, 1500, True), (5, 4, True)))


def _empty_cases():
    s, ids, depth = _scene(3, 3, 100.0, 5, full=False)
    base = _finish(s, ids, depth)
    out = {}
    e = dict(base, point_id=np.zeros(0, np.int64), point_xyz=np.zeros((0, 3), F64), point_error=np.zeros(0, F32))
    out["empty_N"] = e
    out["empty_M"] = dict(base, cam_centers=np.zeros((0, 3), F32), obs_ptr=np.zeros(1, np.int64),
                          obs_point_id=np.zeros(0, np.int64))
    out["empty_O"] = dict(base, obs_ptr=np.zeros(len(base["cam_centers"]) + 1, np.int64),
                          obs_point_id=np.zeros(0, np.int64), runs=((5, 1500, True), (-1, 1500, True)))
    out["empty_D"] = dict(base, depth_centers=None)
    out["empty_D0"] = dict(base, depth_centers=np.zeros((0, 3), F64))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for name, (n_w, n_h, cs, seed) in {"1x1": (1, 1, 100.0, 1), "1x4": (1, 4, 33.3, 2), "4x1": (4, 1, 33.3, 3),
                                       "3x3": (3, 3, 100.0, 4), "3x3_333": (3, 3, 33.3, 6)}.items():
        s, ids, depth = _scene(n_w, n_h, cs, seed)
        out[name] = _finish(s, ids, depth)
    s, ids, depth = _scene(130, 130, 33.3, 9, big=True, full=False)
    out["130x130"] = _finish(s, ids, depth, runs=((5, 1500, True), (0, 1500, True)))
    out["auto"] = _auto_case()
    out.update(_empty_cases())
    # the host thresholds on one scene: max_n_cams below the valid count, min_n_cams equal to the first
    # emitted chunk's count (which excludes it), no far cameras
    first = reference("3x3", (5, 1500, True))["chunks"][0]
    out["3x3"] = dict(out["3x3"], runs=((5, 1500, True), (5, 3, True), (len(first["cameras"]), 1500, True),
                                        (5, 1500, False), (2, 7, True)))
    return out


_BASE = {}


def _case(name):
    """cases()[name], also while cases() itself is being built (the thresholds need a reference)."""
    if name not in _BASE:
        if name == "3x3":
            s, ids, depth = _scene(3, 3, 100.0, 4)
            _BASE[name] = _finish(s, ids, depth)
        else:
            _BASE[name] = cases()[name]
    return _BASE[name]


def grid_of(case):
    if case["grid"] is not None:
        return case["grid"]
    from gs_train.chunker import chunk_grid
    return chunk_grid(case["cam_centers"], case["chunk_size"], 0.2)


@functools.lru_cache(maxsize=None)
def reference(name, run):
    c = _case(name)
    return R.partition(c["cam_centers"], c["obs_ptr"], c["obs_point_id"], c["point_id"], c["point_xyz"],
                       c["point_error"], c["depth_centers"], grid_of(c), c["chunk_size"], min_n_cams=run[0],
                       max_n_cams=run[1], add_far_cams=run[2])


def all_runs():
    return [(name, run) for name, c in cases().items() for run in c["runs"]]
