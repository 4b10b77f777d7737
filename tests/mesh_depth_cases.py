"""Cases of the mesh ray cast and the depth encode (include/gsr_mesh_depth.h): the smallest shapes at
which they can go wrong.  A ray cast case is a dict: name, vertices (V, 3) float32, faces (F, 3) int32,
cams (K, 11) float64 (qvec, tvec, fx, fy, cx, cy), W, H, tnear, tfar, mode, and
    closed   None, or a (K, H, W) bool mask of pixels whose ray cannot miss (from inside a closed
             surface every ray hits: any 0 there is a hole),
    fan      every pixel is judged by the candidate rule (the boundary cap does not apply),
    zero     the whole map is 0, exactly,
    exact    [(k, iy, ix, value)]: pixels whose value is exact (every operation is).
reference(case) is the float64 result per camera (tests/mesh_depth_ref.cast64), computed once and
shared."""
from __future__ import annotations

import functools

import numpy as np

import mesh_depth_ref as R

F32 = np.float32


def rot_to_qvec(Rm):
    """COLMAP qvec (w, x, y, z) of a rotation matrix."""
    t = np.trace(Rm)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = [0.25 * s, (Rm[2, 1] - Rm[1, 2]) / s, (Rm[0, 2] - Rm[2, 0]) / s, (Rm[1, 0] - Rm[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(Rm)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + Rm[i, i] - Rm[j, j] - Rm[k, k]) * 2
        q = [0.0] * 4
        q[0] = (Rm[k, j] - Rm[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (Rm[j, i] + Rm[i, j]) / s
        q[1 + k] = (Rm[k, i] + Rm[i, k]) / s
    return np.array(q, np.float64)


def look_at(eye, target, fx, fy, cx, cy, up=(0.0, 0.0, 1.0)):
    """One camera row: at `eye`, z towards `target`, y down (COLMAP)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rm = np.stack([x, y, z])
    return np.concatenate([rot_to_qvec(Rm), -Rm @ eye, [fx, fy, cx, cy]])


def axis_cam(fx, fy, cx, cy, eye=(0.0, 0.0, 0.0)):
    """Identity rotation: x right, y down, z forward in world axes."""
    return np.concatenate([[1.0, 0, 0, 0], -np.asarray(eye, np.float64), [fx, fy, cx, cy]])


def sheet(nu, nv, size, z, seed, tilt=0.3, jitter=0.3):
    """A jittered, tilted sheet of 2 nu nv triangles around (0, 0, z), facing -z."""
    rng = np.random.default_rng(seed)
    gu, gv = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing="ij")
    u = (gu + rng.uniform(-jitter, jitter, gu.shape)) / nu - 0.5
    v = (gv + rng.uniform(-jitter, jitter, gv.shape)) / nv - 0.5
    w = z + tilt * size * u + 0.02 * size * rng.uniform(-1, 1, gu.shape)
    vert = np.stack([u.reshape(-1) * size, v.reshape(-1) * size, w.reshape(-1)], 1)
    i = (gu[:-1, :-1] * (nv + 1) + gv[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([i, i + nv + 1, i + 1], 1), np.stack([i + 1, i + nv + 1, i + nv + 2], 1)])
    return vert.astype(F32), faces.astype(np.int32)


def icosphere(level, radius, centre=(0.0, 0.0, 0.0)):
    """A closed subdivided icosahedron with every face's vertices duplicated (nothing shared)."""
    p = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p],
                  [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2],
                  [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11],
                  [6, 2, 10], [8, 6, 7], [9, 8, 1]])
    tri = v[f] / np.linalg.norm(v[0])
    for _ in range(level):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = ((x + y) / 2 for x, y in ((a, b), (b, c), (c, a)))
        ab, bc, ca = (x / np.linalg.norm(x, axis=1, keepdims=True) for x in (ab, bc, ca))
        tri = np.concatenate([np.stack(t, 1) for t in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    # (x + y) / 2 and its normalisation are the same numbers whichever face computes them, so the two
    # copies of a shared corner are equal bit for bit
    vert = (tri.reshape(-1, 3) * radius + np.asarray(centre)).astype(F32)
    return vert, np.arange(len(vert), dtype=np.int32).reshape(-1, 3)


def case(name, vertices, faces, cams, W, H, tnear=0.0, tfar=1000.0, mode=0, closed=None, fan=False, zero=False,
         exact=()):
    cams = np.atleast_2d(np.asarray(cams, np.float64))
    return dict(name=name, vertices=np.ascontiguousarray(vertices, F32), faces=np.ascontiguousarray(faces, np.int32),
                cams=cams, W=W, H=H, tnear=tnear, tfar=tfar, mode=mode, closed=closed, fan=fan, zero=zero,
                exact=list(exact))


def _tri(*p):
    return np.array(p, F32), np.array([[0, 1, 2]], np.int32)


def _merge(*meshes):
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs).astype(F32), np.concatenate(fs).astype(np.int32)


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    # ---- sizes and counts
    out.append(case("1x1_F1_K1", *_tri((-3, -3, 5), (3, -3, 5), (0, 4, 6)), axis_cam(1.0, 1.0, 0.5, 0.5), 1, 1))
    quad = (np.array([(-2, -1.5, 6), (2, -1.5, 6.5), (2, 1.5, 7), (-2, 1.5, 6)], F32),
            np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    out.append(case("16x16_F2_K3", *quad, [look_at((e, 0.3, 0), (0, 0, 6), 14, 14, 8, 8, up=(0, -1, 0)) for e in (-1, 0, 1.5)],
                    16, 16))
    ring = [look_at((5 * np.cos(a), 5 * np.sin(a), -1 + 0.03 * k), (0, 0, 6.4), 13, 12, 8.5, 7.5, up=(0, 0, -1))
            for k, a in enumerate(np.linspace(0, 2 * np.pi, 65, endpoint=False))]
    out.append(case("17x15_F2_K65", *quad, ring, 17, 15))
    mid = sheet(12, 25, 9.0, 8.0, seed=3)
    cams3 = [look_at((-2, 0.5, 0), (0, 0, 8), 50, 50, 32, 24, up=(0, -1, 0)),
             look_at((0, 0, 1), (0.5, 0, 8), 40, 60, 30, 20, up=(0, -1, 0)),
             look_at((3, -1, 2), (0, 0, 8), 70, 70, 32, 24, up=(0, -1, 0))]
    out.append(case("64x48_F600_K3", *mid, cams3, 64, 48))
    out.append(case("64x48_F600_K3_z", *mid, cams3, 64, 48, mode=1))
    big = _merge(sheet(32, 64, 14.0, 10.0, seed=5), _tri((-40, -40, 30), (40, -40, 30), (0, 60, 31)))
    assert len(big[1]) == 4097
    out.append(case("130x70_F4097_K1", *big, look_at((1, 0.5, 0), (0, 0, 10), 90, 70, 60, 37, up=(0, -1, 0)), 130, 70))
    # the same scene 2000 m from the origin: the arithmetic runs on differences
    shift = np.array([2000.0, -2000.0, 500.0])
    far = ((mid[0].astype(np.float64) + shift).astype(F32), mid[1])
    out.append(case("shifted_2000m", *far, [look_at(np.array((-2, 0.5, 0)) + shift, np.array((0, 0, 8)) + shift, 50, 50, 32, 24,
                                                    up=(0, -1, 0))], 64, 48))
    # ---- geometry
    small = sheet(3, 3, 2.0, 4.0, seed=7)
    out.append(case("oversize_frame_filling", *_merge(_tri((-300, -300, 50), (300, -300, 50), (0, 400, 50)), small),
                    axis_cam(40, 40, 32, 24), 64, 48))
    out.append(fan_case())
    out.append(case("crossing_camera_plane", *_tri((-4, 1.5, -5), (4, 1.5, -5), (0.5, 1.0, 20)), axis_cam(20, 20, 16, 12), 32, 24))
    out.append(case("crossing_from_the_side", *_tri((-6, -1, -2), (1.5, 0.5, 0.5), (1, 2, 9)), axis_cam(20, 20, 16, 12), 32, 24))
    out.append(case("wholly_behind", *_tri((-4, -4, -5), (4, -4, -5), (0, 4, -1)), axis_cam(8, 8, 8, 8), 16, 16, zero=True))
    # outside each frustum side by more than a pixel: rays at |x / z| <= 7.5 / 8; the triangles start at 9.5 / 8
    z = 8.0
    m = 9.5 / 8 * z
    outside = _merge(_tri((m, -1, z), (m + 3, -1, z), (m, 1, z)), _tri((-m, -1, z), (-m - 3, -1, z), (-m, 1, z)),
                     _tri((-1, m, z), (1, m, z), (0, m + 3, z)), _tri((-1, -m, z), (1, -m, z), (0, -m - 3, z)))
    out.append(case("outside_each_side", *outside, axis_cam(8, 8, 8, 8), 16, 16, zero=True))
    # smaller than a pixel: between centres (misses all), around the centre of pixel (5, 9) (one pixel)
    px = lambda i: (i + 0.5 - 8) / 8 * 4.0  # world x of pixel i's centre on the plane z = 4
    sub = _merge(_tri((px(3) + 0.2, px(3) + 0.2, 4), (px(3) + 0.3, px(3) + 0.2, 4), (px(3) + 0.2, px(3) + 0.3, 4)),
                 _tri((px(9) - 0.1, px(5) - 0.1, 4), (px(9) + 0.15, px(5) - 0.1, 4), (px(9) - 0.1, px(5) + 0.15, 4)))
    out.append(case("subpixel_triangles", *sub, axis_cam(8, 8, 8, 8), 16, 16))
    deg_v = np.array([(0, 0, 4), (1, 0, 4), (1, 0, 4), (2, 2, 4), (-1, -1, 4), (-3, 1, 8), (-1, 1, 8), (1, 1, 8)], F32)
    deg_f = np.array([[0, 1, 2], [3, 3, 3], [0, 3, 4], [5, 6, 7], [0, 1, 1]], np.int32)
    out.append(case("zero_area_and_collinear", deg_v, deg_f, axis_cam(8, 8, 8, 8), 16, 16, zero=True))
    good = sheet(4, 4, 5.0, 6.0, seed=11)
    bad_v = np.concatenate([good[0], np.array([(np.nan, 0, 5), (0, np.inf, 5), (0, 0, 3)], F32)])
    nv = len(good[0])
    bad_f = np.concatenate([good[1], np.array([[0, 1, nv], [nv + 1, 2, 3], [0, 1, nv + 3], [-1, 2, 3], [nv + 2, nv, 4],
                                               [0, 5, 2 ** 31 - 1]], np.int32)])
    out.append(case("non_finite_and_out_of_range", bad_v, bad_f, axis_cam(14, 14, 8, 8), 16, 16))
    co = _merge(_tri((-2, -2, 5), (2, -2, 5.5), (0, 2, 6)), _tri((0, 2, 6), (-2, -2, 5), (2, -2, 5.5)),
                _tri((2, -2, 5.5), (-2, -2, 5), (0, 2, 6)))
    out.append(case("coincident_triangles", *co, axis_cam(14, 14, 8, 8), 16, 16))
    out.append(case("layers_1mm_apart", *_merge(_tri((-9, -9, 5.001), (9, -9, 5.001), (0, 9, 5.001)),
                                                _tri((-9, -8, 5), (9, -8, 5), (0, 9, 5))), axis_cam(14, 14, 8, 8), 16, 16))
    # ---- distance bounds: a power-of-two plane through the one ray (0, 0, 1); every operation is exact
    up1 = lambda x: float(np.nextafter(F32(x), F32(np.inf)))
    plane = lambda zz: _tri((-128, -128, zz), (128, -128, zz), (0, 128, zz))
    one = axis_cam(1.0, 1.0, 0.5, 0.5)
    out.append(case("tfar_exact_hit", *plane(64.0), one, 1, 1, tfar=64.0, exact=[(0, 0, 0, 64.0)]))
    out.append(case("tfar_one_above_miss", *plane(up1(64.0)), one, 1, 1, tfar=64.0, exact=[(0, 0, 0, 0.0)]))
    out.append(case("tnear_exact_miss", *plane(2.0), one, 1, 1, tnear=2.0, exact=[(0, 0, 0, 0.0)]))
    out.append(case("tnear_one_above_hit", *plane(up1(2.0)), one, 1, 1, tnear=2.0, exact=[(0, 0, 0, up1(2.0))]))
    # ---- camera and frame
    out.append(case("principal_point_outside", *small, axis_cam(30, 30, -20.0, 40.0, eye=(-3.7, 4.3, 0)), 16, 16))
    out.append(case("fx_ne_fy_off_centre", *mid, look_at((0, 0, 0), (0, 1, 8), 31, 77, 11.25, 30.5, up=(0, -1, 0)), 48, 40))
    # ---- watertightness
    qv = np.array([(-1, -1, 4), (1, -1, 4), (1, 1, 4), (-1, 1, 4)], F32)
    qf = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    dxy = (np.arange(16) + 0.5 - 8) / 8
    inside = (np.abs(dxy)[None, :] < 0.25) & (np.abs(dxy)[:, None] < 0.25)
    out.append(case("quad_diagonal_through_centres", qv, qf, axis_cam(8, 8, 8, 8), 16, 16, closed=inside[None]))
    ico = icosphere(2, 3.0)
    icams = [look_at((0, 0, 0), (1, 0.2, 0.1), 20, 20, 32, 24), look_at((0.8, -0.5, 0.4), (-1, 1, 0.3), 9, 14, 30, 20),
             look_at((0, 0, 0), (0, 0, 1), 24, 24, 32, 24, up=(0, 1, 0))]
    out.append(case("icosphere_from_inside", *ico, icams, 64, 48, closed=np.ones((3, 48, 64), bool)))
    return out


def fan_case():
    """5000 slivers around one apex, all inside one 16 x 16 tile of a 32 x 32 frame: more than one LDS
    batch for that tile."""
    n, zc = 5000, 4.0
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
    apex = np.array([[0.6, 0.55, zc]])
    rim = np.stack([0.6 + 0.4 * np.cos(ang), 0.55 + 0.4 * np.sin(ang), zc + 0.5 * np.sin(3 * ang)], 1)
    vert = np.concatenate([apex, rim]).astype(F32)
    i = np.arange(n)
    faces = np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1).astype(np.int32)
    # fx = 48, z = 3.5 .. 4.5: the fan's grown bounds stay inside pixels 16 .. 31, the tile (1, 1)
    return case("fan_5000_in_one_tile", vert, faces, axis_cam(48, 48, 16, 16), 32, 32, fan=True)


NAMES = [c["name"] for c in all_cases()]


def by_name(name):
    return all_cases()[NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def reference(name):
    """[cast64 result per camera] of a case."""
    c = by_name(name)
    return [R.cast64(c["vertices"], c["faces"], cam, c["W"], c["H"], c["tnear"], c["tfar"], c["mode"])
            for cam in c["cams"]]


# ---- encode inputs: authored distance maps ------------------------------------------------------------

def encode_cases():
    """[(name, distance (K, H, W) float32, kwargs)]."""
    f = F32
    out = []
    edges = []
    for m in (0.001, 65.536, 262.144, 1048.576):
        x = f(m)
        edges += [np.nextafter(x, f(0)), x, np.nextafter(x, f(np.inf))]
        # float32 neighbours of the metres value whose mm product lies on either side of the limit
    mm_exact = [f(v) for v in (0.004, 0.1, 0.25, 1.0, 2.5, 64.0, 65.5, 66.0, 70.0, 256.0, 262.0, 263.0, 300.0, 1024.0, 1048.0,
                               1049.0, 2000.0)]
    row = np.array(edges + mm_exact + [f(0), f(np.nan), f(-1.0), f(np.inf)], f)
    out.append(("code_limits", np.tile(row, (3, 1))[None], {}))
    out.append(("code_limits_unquantized", np.tile(row, (3, 1))[None], {"quantize": False}))
    md = np.array([np.nextafter(f(0.1), f(0)), f(0.1), np.nextafter(f(0.1), f(1)), 0.104, 0.108, 5.0,
                   np.nextafter(f(50.0), f(0)), 50.0, np.nextafter(f(50.0), f(100)), 49.9, 50.1], f)
    out.append(("min_and_max_depth", md[None, None], {"max_depth": 50.0}))
    out.append(("min_and_max_depth_unquantized", md[None, None], {"max_depth": 50.0, "quantize": False}))
    out.append(("all_background", np.zeros((2, 5, 7), f), {}))
    one = np.zeros((1, 4, 6), f)
    one[0, 2, 3] = 7.3
    out.append(("one_valid_pixel", one, {}))
    two = np.zeros((1, 4, 6), f)
    two[0, 1, 1] = two[0, 3, 5] = 12.345
    out.append(("two_equal_valid_pixels", two, {}))
    out.append(("one_pixel_map", np.full((1, 1, 1), 3.0, f), {}))
    rng = np.random.default_rng(17)
    big = np.exp(rng.uniform(np.log(0.05), np.log(1200.0), (2, 70, 130))).astype(f)
    big[rng.uniform(size=big.shape) < 0.2] = 0
    out.append(("130x70", big, {}))
    out.append(("130x70_unquantized", big, {"quantize": False, "min_depth": 0.5, "max_depth": 300.0}))
    many = np.exp(rng.uniform(np.log(0.2), np.log(90.0), (65, 9, 11))).astype(f)
    many[rng.uniform(size=many.shape) < 0.3] = 0
    many[7] = 0  # an image without a valid pixel in the middle of the batch
    many[9] = 4.0  # and one of equal pixels
    out.append(("K65", many, {}))
    return out
