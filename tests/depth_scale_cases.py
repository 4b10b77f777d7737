"""The depth scale fit's cases: the smallest inputs at which each part of the rule (gsr_depth_scale.h) and
of the kernel (csrc/depth_scale.hip) can go wrong.  Maps 6 x 8 to 48 x 64, cameras up to 96 x 64,
s = Hd / height of 1, 1/2, 2 and 1/3.

A scene is one call: dict(name, Hd, Wd, point_id, point_xyz, images); an image is dict(name, q, t, width,
height, xy, pid, u16 or None).  Cameras sit at identity or at rotations of entries 0, +-1 with t on a
coarse grid, points on a 2^-8 grid, so z is exact and no observation or image is one fp64 could decide
either way (tests/test_depth_scale_cpu.py checks the margins in extended precision).
reference(name, missing) is the restatement's answer per image, computed once."""
from __future__ import annotations

import functools

import numpy as np

import depth_scale_ref as R

I4 = (1.0, 0.0, 0.0, 0.0)
MODES = ("origin", "skip")


def capacity() -> int:
    """C: the kernel's LDS capacity in observations."""
    from diff_gaussian_rasterization import _lib
    return int(_lib.load().gsr_depth_scale_lds_capacity())


def _table(rng, n_front=48):
    """Ids 3 k + 1 (gaps at 3 k and 3 k + 2): n_front points in front of an identity camera at the
    origin, then row n_front: z = the smallest double >= 1e-6; n_front + 1: z = -5 (behind); n_front + 2: a NaN point."""
    xyz = np.round(np.stack([rng.uniform(-4, 4, n_front), rng.uniform(-3, 3, n_front),
                             rng.uniform(2, 30, n_front)], 1) * 256) / 256
    xyz = np.concatenate([xyz, [[0.0, 0.0, np.nextafter(1e-6, 1.0)], [0.5, 0.25, -5.0], [np.nan, 1.0, 4.0]]])
    ids = 3 * np.arange(len(xyz), dtype=np.int64) + 1
    perm = rng.permutation(len(xyz))  # rows in no particular order
    return ids[perm], xyz[perm], ids[:n_front], ids[n_front], ids[n_front + 1], ids[n_front + 2]


def _noise_map(rng, Hd, Wd):
    return rng.integers(0, 65536, (Hd, Wd)).astype(np.uint16)


def _image(name, xy, pid, u16, width, height, q=I4, t=(0.0, 0.0, 0.0)):
    return dict(name=name, q=np.asarray(q, np.float64), t=np.asarray(t, np.float64), width=int(width), height=int(height),
                xy=np.asarray(xy, np.float64).reshape(-1, 2), pid=np.asarray(pid, np.int64).reshape(-1), u16=u16)


def _inside(rng, n, width, height):
    return np.stack([rng.uniform(0.5, width - 1.5, n), rng.uniform(0.5, height - 1.5, n)], 1)


def _counts_scene(C):
    """Observation counts per image (every observation valid unless said): around the acceptance
    threshold, the wave (64), the workgroup (256) and the LDS capacity C."""
    rng = np.random.default_rng(2401)
    ids, xyz, front, tiny, behind, nanp = _table(rng)
    W, H, Hd, Wd = 64, 48, 24, 32  # s = 1 / 2
    imgs = []
    imgs.append(_image("n0", np.zeros((0, 2)), np.zeros(0, np.int64), _noise_map(rng, Hd, Wd), W, H))
    imgs.append(_image("all_minus_one", _inside(rng, 40, W, H), np.full(40, -1), _noise_map(rng, Hd, Wd), W, H))
    for n in (10, 11, 12, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 3 * C + 5):
        imgs.append(_image(f"n{n}", _inside(rng, n, W, H), rng.choice(front, n), _noise_map(rng, Hd, Wd), W, H))
    # the same thresholds with invalid observations in between: the compaction has gaps to close
    for n in (10, 11, 257, C + 1):
        m = n + n // 2 + 3
        pid = rng.choice(front, m)
        xy = _inside(rng, m, W, H)
        bad = rng.permutation(m)[:m - n]
        kinds = np.arange(len(bad)) % 4
        pid[bad[kinds == 0]] = -1
        pid[bad[kinds == 1]] = behind
        xy[bad[kinds == 2], 0] = -1.0
        xy[bad[kinds == 3], 1] = float(H)
        imgs.append(_image(f"n{n}_of_{m}", xy, pid, _noise_map(rng, Hd, Wd), W, H))
    return dict(name="counts", Hd=Hd, Wd=Wd, point_id=ids, point_xyz=xyz, images=imgs)


def _positions_scene(s_name, W, H, Hd, Wd, seed):
    """Map positions at the edges of validity and of the sample: the base observations make the image
    fitted, the special ones move s_mono if they are taken, sampled or rounded differently."""
    rng = np.random.default_rng(seed)
    ids, xyz, front, tiny, behind, nanp = _table(rng)
    s = Hd / H
    bw, bh = np.float32(W * s), np.float32(H * s)
    below_w = float(np.nextafter(bw, np.float32(0))) / s  # maps (after one rounding) to the largest fp32 < bw
    below_h = float(np.nextafter(bh, np.float32(0))) / s
    at_w, at_h = float(bw) / s, float(bh) / s

    def img(name, special):
        special = np.asarray(special, np.float64).reshape(-1, 2)
        xy = np.concatenate([_inside(rng, 14, W, H), special])
        return _image(name, xy, rng.choice(front, len(xy)), _noise_map(rng, Hd, Wd), W, H)

    ties = [((k + 0.5) / 32 / s, (k2 + 0.5) / 32 / s) for k, k2 in ((64, 33), (65, 34), (130, 131), (37, 36))]
    imgs = [
        img("zero_corner", [[0.0, 0.0], [-0.0, 3.0], [3.0, -0.0], [-0.0, -0.0]]),
        img("just_outside", [[-1e-9, 3.0], [3.0, -1e-9], [at_w, 3.0], [3.0, at_h], [float(W), 3.0], [3.0, float(H)]]),
        img("just_inside", [[below_w, 3.0], [3.0, below_h], [below_w, below_h]]),
        img("ties_even_and_odd", ties),
        img("last_row_and_column", [[(Wd - 1) / s, 2.0], [(Wd - 0.5) / s, 2.0], [2.0, (Hd - 1) / s], [2.0, (Hd - 0.25) / s],
                                    [(Wd - 0.5) / s, (Hd - 0.5) / s]]),
        img("nan_and_inf", [[np.nan, 3.0], [3.0, np.nan], [np.inf, 3.0], [3.0, np.inf], [-np.inf, 3.0], [3.0, -np.inf]]),
    ]
    return dict(name=f"positions_s{s_name}", Hd=Hd, Wd=Wd, point_id=ids, point_xyz=xyz, images=imgs)


def bound_rounds_down(W, H, Hd):
    """fl32(width s) < width s in fp64: an fp32 position at the fp32 bound passes an fp64 comparison."""
    s = Hd / H
    return float(np.float32(W * s)) < W * s


def _range_z(rel):
    """z < 0 with inv = 5e-4 - 1e-3 (1 + rel): against valid inverse depths of 5e-4 the range is 1e-3 (1 + rel)."""
    return 1.0 / (5e-4 - 1e-3 * (1.0 + rel))


def _depths_scene():
    """Depths, ids and maps.  6 x 8 map, 16 x 12 camera (s = 1 / 2), identity camera at the origin."""
    rng = np.random.default_rng(2403)
    ids, xyz, front, tiny, behind, nanp = _table(rng)
    # three more rows: z = 2000 (inv = 5e-4) and the two points behind the camera that put the range on
    # either side of 1e-3
    far_id, lo_id, hi_id = int(ids.max()) + 3, int(ids.max()) + 6, int(ids.max()) + 9
    xyz = np.concatenate([xyz, [[0.0, 0.0, 2000.0], [0.0, 0.0, _range_z(-1.001e-6)], [0.0, 0.0, _range_z(1.001e-6)]]])
    ids = np.concatenate([ids, [far_id, lo_id, hi_id]])
    W, H, Hd, Wd = 16, 12, 6, 8
    T = int(ids.max()) + 1
    gap_ids = np.array([0, 2, 3, 5], np.int64)  # ids below T without a row
    flat = np.full((Hd, Wd), 777, np.uint16)
    two = np.where(np.arange(Hd * Wd).reshape(Hd, Wd) % 2 == 0, 1000, 50000).astype(np.uint16)
    extremes = np.where(rng.integers(0, 2, (Hd, Wd)) == 0, 0, 65535).astype(np.uint16)
    # six observations on map pixel (2, 2) (even: 1000) and six on (2, 3) (odd: 50000): the median is between
    on_two = np.stack([np.where(np.arange(12) < 6, 4.0, 6.0), np.full(12, 4.0)], 1)

    def img(name, pid, u16=None, xy=None, flat_map=False, t=(0.0, 0.0, 0.0)):
        pid = np.asarray(pid, np.int64)
        u = flat if flat_map else (_noise_map(rng, Hd, Wd) if u16 is None else u16)
        return _image(name, _inside(rng, len(pid), W, H) if xy is None else xy, pid, u, W, H, t=t)

    base = lambda n: rng.choice(front, n)
    imgs = [
        img("behind_camera", np.concatenate([base(13), [behind] * 3])),
        img("z_1e-6", np.concatenate([base(13), [tiny]])),
        img("equal_depths_odd", np.concatenate([base(4), [front[0]] * 9])),      # the median sits in a run of ties
        img("equal_depths_even", np.concatenate([base(5), [front[1]] * 9])),
        img("range_below_1e-3", np.concatenate([[far_id] * 12, [lo_id]]), flat_map=True),   # not fitted: 0, 0
        img("range_above_1e-3", np.concatenate([[far_id] * 12, [hi_id]]), flat_map=True),   # fitted: 0 / 0
        img("range_from_valid_only_is_zero", np.concatenate([[far_id] * 12, [hi_id]])),     # fitted, s_colmap = 0
        img("ids_at_and_above_T", np.concatenate([base(12), [T, T + 1, 2 ** 31, 2 ** 40, -1, -7]])),
        img("ids_in_gaps", np.concatenate([base(12), gap_ids])),
        img("only_gaps_and_ten", np.concatenate([base(10), gap_ids[:2]])),   # origin: z = t2 = 4, 12 valid; skip: 10
        img("nan_point", np.concatenate([base(14), [nanp]])),
        img("flat_map", base(15), flat_map=True),
        img("two_valued_tie_at_median", base(12), u16=two, xy=on_two),
        img("zero_and_65535", base(17), u16=extremes),
        img("absent_map", base(15)),
        img("turned_round", base(20)),
    ]
    imgs[9]["t"] = np.array([0.0, 0.0, 4.0])      # an origin point is in front of this camera
    imgs[8]["t"] = np.array([0.0, 0.0, 0.25])     # origin points at z = 0.25: valid, far from the others
    imgs[14]["u16"] = None
    imgs[15]["q"] = np.array([0.0, 1.0, 0.0, 0.0])  # R = diag(1, -1, -1): every point behind
    return dict(name="depths_ids_maps", Hd=Hd, Wd=Wd, point_id=ids, point_xyz=xyz, images=imgs)


@functools.lru_cache(maxsize=None)
def scenes():
    out = [_counts_scene(capacity()), _depths_scene(),
           _positions_scene("1", 64, 48, 48, 64, 2411), _positions_scene("1_2", 96, 64, 32, 48, 2412),
           _positions_scene("2", 24, 16, 32, 48, 2413), _positions_scene("1_3", 92, 63, 21, 31, 2414)]
    assert bound_rounds_down(92, 63, 21)
    return out


def by_name(name):
    return next(sc for sc in scenes() if sc["name"] == name)


@functools.lru_cache(maxsize=None)
def reference(name, missing="origin"):
    sc = by_name(name)
    return [R.fit_image(im["q"], im["t"], im["width"], im["height"], im["xy"], im["pid"], sc["point_id"],
                        sc["point_xyz"], im["u16"], missing) for im in sc["images"]]


def arrays(sc):
    """The scene as fit_depth_scales takes it: qvecs, tvecs, sizes, obs_ptr, obs_xy, obs_point_id, maps
    (K, Hd, Wd) uint16 and map_index (-1 for an image without a map)."""
    ims = sc["images"]
    q, t = np.stack([im["q"] for im in ims]), np.stack([im["t"] for im in ims])
    sizes = np.array([[im["width"], im["height"]] for im in ims], np.int64)
    ptr = np.concatenate([[0], np.cumsum([len(im["pid"]) for im in ims])]).astype(np.int64)
    xy = np.concatenate([im["xy"] for im in ims])
    pid = np.concatenate([im["pid"] for im in ims])
    with_map = [k for k, im in enumerate(ims) if im["u16"] is not None]
    maps = np.stack([ims[k]["u16"] for k in with_map])
    index = np.full(len(ims), -1, np.int64)
    index[with_map] = np.arange(len(with_map))
    return q, t, sizes, ptr, xy, pid, maps, index
