"""Needles, discs, points, reset and faint splats for the parity tests (test_oracle.py,
test_gpu_shapes.py): the shapes a trained street chunk is made of and gs_oracle.synthetic_scene
never draws (its three log-scales come from one normal with std 0.5, its opacities from
[0.05, 0.99]).  Inputs, row masks and population checks only: nothing here asserts anything
about the code under test.

`populate_shapes` rewrites a share of the rows of a camera-space scene (before
posed_cases.pose_scene):
  needle  one long axis, two at 1e-3; the long axis' on-screen sigma log-uniform in `px`; 40 % of
          them lie in the image plane within 1 degree of the screen x axis, the y axis or a
          diagonal, the rest are turned at random and tilted up to 60 degrees out of the plane;
  disc    two long axes, one at 1e-3; half with the thin axis within 10 degrees of the ray to the
          camera (face-on), half with it within 0.5 degrees of perpendicular to the ray (edge-on:
          the projection is a line);
  point   all three axes 1e-7: the 2D covariance is 0.3 I to fp32;
  reset   opacity exactly float32(0.01), the value an opacity reset leaves;
  faint   opacities at float32(1/255) and its two float neighbours (rows whose 2D means are then
          moved exactly onto pixel centres near the frame's middle, under the camera the scene has
          at that moment), the rest uniformly below 1/255.
`shape_subsets` gives the row masks (from the oracle's forward state), `assert_shapes_populated`
fails a case whose claimed population is not there.

`single_frame` builds the one-splat frames of the alpha-map tests and `alpha_map_check` compares
such a frame's blend decisions and alphas with fp64, given the rounding band of the quadratic form
(`band`).
"""
from __future__ import annotations

import math

import numpy as np

THIN = np.float32(1e-3)
POINT = np.float32(1e-7)
RESET = np.float32(0.01)
THRESH = np.float32(1.0 / 255.0)       # the blend's alpha threshold, as the kernels compare it
CAP = np.float32(0.99)
MIN_THIN, MIN_THIN_LONG, MIN_POINT, MIN_RESET, MIN_FAINT = 100, 30, 200, 100, 50
ALIGNED_SHARE = 0.4


def _quat(R):
    """Rotation matrix (columns = axes) -> quaternion (r, x, y, z), the rasterizer's order."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        q = (0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s)
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2]) * 2
        q = ((R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s)
    elif R[1, 1] > R[2, 2]:
        s = math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2]) * 2
        q = ((R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s)
    else:
        s = math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1]) * 2
        q = ((R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s)
    return np.array(q)


def _rotation(q):
    """Unit quaternion (r, x, y, z) -> rotation matrix."""
    r, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def _frame(n, h):
    """Right-handed orthonormal axes (n, u, v) with u = h made perpendicular to n."""
    n = n / np.linalg.norm(n)
    u = h - np.dot(h, n) * n
    u /= np.linalg.norm(u)
    return np.stack([n, u, np.cross(n, u)], 1)


def needle_rotation(theta_deg, phi_deg=0.0):
    """Quaternion whose first axis is (cos t cos p, sin t cos p, sin p): in the image plane of the
    identity camera at angle t to the screen x axis, tilted p out of it."""
    t, p = math.radians(theta_deg), math.radians(phi_deg)
    d = np.array([math.cos(t) * math.cos(p), math.sin(t) * math.cos(p), math.sin(p)])
    return _quat(_frame(d, np.array([0.0, 0.0, 1.0]) if abs(d[2]) < 0.9 else np.array([1.0, 0.0, 0.0])))


def _ray_frame(m):
    r = m / np.linalg.norm(m)
    t1 = np.cross([0.0, 1.0, 0.0], r)
    t1 /= np.linalg.norm(t1)
    return r, t1, np.cross(r, t1)


def disc_rotation(mean, edge_on, psi_deg, tilt_deg):
    """Quaternion whose first (thin) axis is, face-on, the ray to `mean` tilted by tilt_deg towards
    the in-plane direction psi, and edge-on the in-plane direction psi tilted by tilt_deg towards
    the ray.  Camera space of a camera at the origin."""
    r, t1, t2 = _ray_frame(np.asarray(mean, np.float64))
    psi, tilt = math.radians(psi_deg), math.radians(tilt_deg)
    inplane = math.cos(psi) * t1 + math.sin(psi) * t2
    if edge_on:
        return _quat(_frame(math.cos(tilt) * inplane + math.sin(tilt) * r, r))
    return _quat(_frame(math.cos(tilt) * r + math.sin(tilt) * inplane, t1))


def project(s, idx):
    """The oracle's 2D means of rows idx of scene s (its fp32 preprocess)."""
    import gs_oracle as O
    idx = np.atleast_1d(idx)
    st = O.forward(s["means3D"][idx], np.full(len(idx), 0.5, np.float32), s["view"], s["proj"], s["campos"], s["bg"],
                   s["W"], s["H"], s["tanfovx"], s["tanfovy"], sh_degree=0, colors_precomp=np.ones((len(idx), 3)),
                   scales=np.full((len(idx), 3), 1e-7, np.float32),
                   rotations=np.tile(np.float32([1, 0, 0, 0]), (len(idx), 1)))
    return st["xy"].astype(np.float64)


def _snap(s, i, target):
    m = s["means3D"]
    fx, fy = s["W"] / (2.0 * s["tanfovx"]), s["H"] / (2.0 * s["tanfovy"])
    xy = project(s, i)[0]
    for _ in range(4):
        m[i, 0] = np.float32(m[i, 0] + (target[0] - xy[0]) * m[i, 2] / fx)
        m[i, 1] = np.float32(m[i, 1] + (target[1] - xy[1]) * m[i, 2] / fy)
        xy = project(s, i)[0]
    for ax in (0, 1):
        for _ in range(64):
            if xy[ax] == target[ax]:
                break
            m[i, ax] = np.nextafter(m[i, ax], np.float32(np.inf if xy[ax] < target[ax] else -np.inf))
            xy = project(s, i)[0]
    return np.array_equal(xy, target)


def snap_to_pixel(s, i, target):
    """Move row i's mean (x and y of the camera-space point, identity view) until its fp32 2D mean
    is exactly `target`.  Targets belong near the frame's middle: towards an edge the fp32 pixel
    coordinate ((ndc + 1) W - 1) / 2 steps by 1e-5 px and can miss an integer.  In place."""
    target = np.asarray(target, np.float64)
    assert _snap(s, i, target), ("no float mean projects onto", target)
    return target


def populate_shapes(s, seed, needle=0.0, disc=0.0, point=0.0, reset=0.0, faint=0.0, px=(8.0, 80.0)):
    """The shape populations, on a scene still in camera space (before pose_scene).  `needle`, `disc`
    and `point` are disjoint shares of the rows; `reset` and `faint` are shares of all rows, drawn
    independently of the shape (faint wins over reset).  px: the on-screen long sigma's range in
    pixels.  In place; s["shape_rows"] keeps the row indices of each population."""
    P = s["means3D"].shape[0]
    rng = np.random.default_rng(seed + 401)
    m = s["means3D"].astype(np.float64)
    z = m[:, 2]
    fx = s["W"] / (2.0 * s["tanfovx"])
    u = rng.random(P)
    rows = dict(needle=np.nonzero(u < needle)[0], disc=np.nonzero((u >= needle) & (u < needle + disc))[0],
                point=np.nonzero((u >= needle + disc) & (u < needle + disc + point))[0])
    lo, hi = math.log(px[0]), math.log(px[1])
    for i in rows["needle"]:
        sigma = math.exp(rng.uniform(lo, hi))
        if rng.random() < ALIGNED_SHARE:
            theta, phi = float(rng.choice([0.0, 90.0, 45.0, 135.0])) + rng.uniform(-1.0, 1.0), 0.0
        else:
            theta, phi = rng.uniform(0.0, 180.0), rng.uniform(-60.0, 60.0)
        s["rotations"][i] = needle_rotation(theta, phi).astype(np.float32)
        s["scales"][i] = (np.float32(sigma * z[i] / (fx * math.cos(math.radians(phi)))), THIN, THIN)
    for k, i in enumerate(rows["disc"]):
        edge_on = bool(k & 1)
        tilt = rng.uniform(-0.5, 0.5) if edge_on else rng.uniform(0.0, 10.0)
        s["rotations"][i] = disc_rotation(m[i], edge_on, rng.uniform(0.0, 360.0), tilt).astype(np.float32)
        s1, s2 = (math.exp(rng.uniform(lo, hi)) * z[i] / fx for _ in range(2))
        s["scales"][i] = (THIN, np.float32(s1), np.float32(s2))
    s["scales"][rows["point"]] = POINT
    if reset:
        rows["reset"] = np.nonzero(rng.random(P) < reset)[0]
        s["opacities"][rows["reset"]] = RESET
    if faint:
        f = np.nonzero(rng.random(P) < faint)[0]
        assert len(f) >= 3
        op = rng.uniform(0.0, float(THRESH), len(f)).astype(np.float32)
        op[op >= THRESH] = np.float32(0.0)
        op[:3] = (THRESH, np.nextafter(THRESH, np.float32(1)), np.nextafter(THRESH, np.float32(0)))
        s["opacities"][f, 0] = op
        for k, i in enumerate(f[:3]):
            snap_to_pixel(s, i, (s["W"] // 2 + 3 + 5 * k, s["H"] // 2 + 1 + 3 * k))
        rows["faint"], rows["threshold"] = f, f[:3]
    s["shape_rows"] = rows
    return s


def make_scene(c):
    """A case dict of test_gpu_parity.make_scene plus pose (posed_cases) and the shape shares
    needle / disc / point / reset / faint with their pixel range px."""
    import posed_cases as PC
    from test_gpu_parity import make_scene as base_scene
    name = c.get("pose", "identity")
    p = None
    if name != "identity":
        p = PC.pose(name, c["W"], c["H"])
        c = dict(c, fovx=p["fovx_deg"])
    s = base_scene(c)
    populate_shapes(s, c["seed"], **{k: c[k] for k in ("needle", "disc", "point", "reset", "faint", "px") if k in c})
    if p is None:
        return s
    # pose_scene moves the means alone, which is enough for round blobs; a needle's or a disc's axes
    # have to turn with the world as well, or the posed camera sees another shape
    V3 = p["view"].astype(np.float64).reshape(4, 4)[:3, :3]   # camera-space axis -> world: V3 @ axis
    for i in np.concatenate([s["shape_rows"]["needle"], s["shape_rows"]["disc"]]):
        s["rotations"][i] = _quat(V3 @ _rotation(s["rotations"][i].astype(np.float64))).astype(np.float32)
    return PC.pose_scene(s, p)


def conic_axes(co):
    """(eigenvalue ratio of the 2D covariance, long sigma in pixels) from stored conics, fp64."""
    a, b, c = (co[:, k].astype(np.float64) for k in range(3))
    mid, det = 0.5 * (a + c), a * c - b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        lmax = mid + np.sqrt(np.maximum(mid * mid - det, 0.0))
        lmin = det / lmax                      # the conic's small eigenvalue: 1 / long sigma^2
        return lmax / lmin, 1.0 / np.sqrt(lmin)


def shape_subsets(s, st):
    """Row masks from the oracle's forward state `st` of scene `s`:
      thin       visible, eigenvalue ratio of the 2D covariance (from the stored conic, fp64) >= 100;
      thin_long  thin and long sigma >= 30 px;
      point      visible and radii <= 3;
      reset      opacity == float32(0.01);
      faint      opacity < float32(1/255);
    and `visible`, `touched` (tiles_touched > 0), `on_centre` (the 2D mean is a pixel centre)."""
    vis = (st["radii"] > 0) & (st["tiles_touched"] > 0)
    ratio, sigma = conic_axes(st["conic_opacity"])
    with np.errstate(invalid="ignore"):
        thin = vis & (ratio >= 100.0)
        thin_long = thin & (sigma >= 30.0)
    op = np.asarray(s["opacities"], np.float32).reshape(-1)
    xy = st["xy"]
    return dict(thin=thin, thin_long=thin_long, point=vis & (st["radii"] <= 3), reset=op == RESET, faint=op < THRESH,
                visible=vis, touched=st["tiles_touched"] > 0, on_centre=np.all(xy == np.rint(xy), axis=1))


CLAIM_SUBSETS = dict(thin=("thin", "thin_long"), point=("point",), reset=("reset",), faint=("faint",))


def claimed_subsets(c):
    return tuple(n for k in c["claims"] for n in CLAIM_SUBSETS[k])


def assert_shapes_populated(masks, grads, claimed=("thin", "point", "reset", "faint"), rows=None):
    """Every population a case claims is there (`grads`: the oracle's backward; `rows`: the scene's
    shape_rows, for the three threshold rows of a faint population)."""
    moved = np.any(grads["dL_dmeans3D"] != 0, axis=1)
    if "thin" in claimed:
        n, nl = int((masks["thin"] & moved).sum()), int((masks["thin_long"] & moved).sum())
        assert n >= MIN_THIN and nl >= MIN_THIN_LONG, ("thin / thin_long rows with a position gradient", n, nl)
    if "point" in claimed:
        n = int((masks["point"] & moved).sum())
        assert n >= MIN_POINT, ("point rows with a position gradient", n, int(masks["point"].sum()))
    if "reset" in claimed:
        n = int((masks["reset"] & moved).sum())
        assert n >= MIN_RESET, ("reset rows with a position gradient", n, int(masks["reset"].sum()))
    if "faint" in claimed:
        n = int((masks["faint"] & masks["touched"]).sum())
        assert n >= MIN_FAINT, ("faint rows that touch a tile", n)
        if rows is not None:
            t = rows["threshold"]
            assert masks["on_centre"][t].all() and masks["touched"][t].all(), "threshold rows off their pixel centres"
            assert list(masks["faint"][t]) == [False, False, True]


# ------------------------------------------------------------------------------------------------
# One-splat frames: the image is the splat's alpha map
# ------------------------------------------------------------------------------------------------
Z0 = 5.0
OPACITIES = dict(o99=np.float32(0.99), o01=RESET, thr=THRESH, thr_up=np.nextafter(THRESH, np.float32(1)),
                 thr_dn=np.nextafter(THRESH, np.float32(0)))


def single_frame(shape, sigma, angle, centre, opacity, W=None, H=None):
    """One Gaussian under the identity camera with colour 1 on black.
    shape: needle | edge_disc | face_disc | point; sigma: on-screen long sigma in px; angle: of the
    long axis to the screen x axis, degrees; centre: pixel (a pixel centre, exactly) | corner (a
    tile corner, between four pixels) | sbrow (the first pixel row of a 16x4 sub-block, y = 4k
    exactly) | off (200 px outside the frame, back along the long axis from the frame's middle)."""
    import gs_oracle as O
    W, H = (W, H) if W else ((1920, 1080) if sigma >= 400 else (640, 480))
    s = O.synthetic_scene(1, W, H, seed=0, sh_degree=0)
    s["bg"] = np.zeros(3, np.float32)
    s["opacities"] = np.full((1, 1), OPACITIES[opacity], np.float32)
    fx, fy = W / (2.0 * s["tanfovx"]), H / (2.0 * s["tanfovy"])
    cx, cy = W // 2 + 3, H // 2 + 1
    if centre == "corner":
        target = (16 * (cx // 16) - 0.5, 16 * (cy // 16) - 0.5)
    elif centre == "sbrow":
        target = (cx + 0.37, 4 * (cy // 4))
    elif centre == "off":
        ux, uy = math.cos(math.radians(angle)), math.sin(math.radians(angle))
        tx = (cx + 200.0) / ux if ux > 1e-9 else math.inf
        ty = (cy + 200.0) / uy if uy > 1e-9 else math.inf
        t = min(tx, ty)
        target = (cx - t * ux, cy - t * uy)
    else:
        target = (cx, cy)
    s["means3D"][0] = (np.float32((target[0] - (W - 1) / 2.0) * Z0 / fx), np.float32((target[1] - (H - 1) / 2.0) * Z0 / fy),
                       np.float32(Z0))
    if centre == "pixel":
        snap_to_pixel(s, 0, target)
    elif centre == "sbrow":
        snap_to_pixel(s, 0, (project(s, 0)[0][0], target[1]))
    long_ = np.float32(sigma * Z0 / fx)
    if shape == "needle":
        s["rotations"][0] = needle_rotation(angle).astype(np.float32)
        s["scales"][0] = (long_, THIN, THIN)
    elif shape == "edge_disc":   # thin axis in the image plane, perpendicular to `angle`; one long axis on the ray
        s["rotations"][0] = disc_rotation(s["means3D"][0], True, angle + 90.0, 0.2).astype(np.float32)
        s["scales"][0] = (THIN, long_, long_)
    elif shape == "face_disc":   # second long axis a quarter of the first: an ellipse at `angle`
        r, t1, t2 = _ray_frame(s["means3D"][0].astype(np.float64))
        a = math.radians(angle)
        s["rotations"][0] = _quat(_frame(r, math.cos(a) * t1 + math.sin(a) * t2)).astype(np.float32)
        s["scales"][0] = (THIN, long_, np.float32(0.25) * long_)
    elif shape == "point":
        s["scales"][0] = POINT
    else:
        raise ValueError(shape)
    return s


def frame_name(f):
    return "_".join(str(v) for v in f)


def _frames():
    F = []
    for sigma in (10, 100, 400):                      # every length at every orientation
        for angle in (0, 1, 45, 89, 90):
            F.append(("needle", sigma, angle, "pixel", "o99"))
    for sigma in (100, 400):                          # centres, and the opacities that shrink the core
        for angle in (1, 89):
            F += [("needle", sigma, angle, c, "o99") for c in ("corner", "sbrow")]
        for angle in (0, 1, 45, 89, 90) if sigma == 400 else (0, 90):
            F.append(("needle", sigma, angle, "off", "o99"))
        F += [("needle", sigma, 1 if sigma == 400 else 45, "pixel", o) for o in ("o01", "thr", "thr_up", "thr_dn")]
    for sigma in (10, 100, 400):
        F += [("edge_disc", sigma, angle, "pixel", "o99") for angle in (0, 1, 45)]
    F += [("edge_disc", 400, 89, "off", "o99"), ("edge_disc", 100, 1, "corner", "o01")]
    F += [("face_disc", 10, 45, "pixel", "o99"), ("face_disc", 100, 1, "corner", "o99"),
          ("face_disc", 100, 89, "sbrow", "o01"), ("face_disc", 400, 45, "pixel", "o99")]
    F += [("point", 0, 0, c, "o99") for c in ("pixel", "corner", "sbrow")]
    F += [("point", 0, 0, "pixel", o) for o in ("o01", "thr", "thr_up", "thr_dn")]
    return F


FRAMES = _frames()


def rect_mask(xy, radius, W, H):
    """Pixels of the tiles in the splat's tile rectangle (the rasterizer's getRect, fp32)."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    x, y, r = np.float32(xy[0]), np.float32(xy[1]), np.float32(radius)
    f = lambda v, g: min(g, max(0, int(np.float32(v) / np.float32(16))))
    x0, x1 = f(x - r, gx), f(x + r + np.float32(15), gx)
    y0, y1 = f(y - r, gy), f(y + r + np.float32(15), gy)
    m = np.zeros((H, W), bool)
    m[16 * y0:16 * y1, 16 * x0:16 * x1] = True
    return m


def band(xy, co, W, H):
    """fp64 quantities of one splat over the frame, from its stored record (2D mean, conic, opacity):
      Q      a dx^2 + 2 b dx dy + c dy^2 at every pixel centre;
      tau    2 ln(opacity / float32(1/255)): alpha >= 1/255  <=>  Q <= tau;
      gamma  2^-21 (a dx^2 + 2 |b dx dy| + c dy^2) + 2^-22 tau, a bound on the fp32 rounding of Q:
             three products and two sums of terms of that size, each within 2^-24 relative, with
             room for the rounding of dx, dy and the scaled conic;
      alpha  min(0.99, opacity exp(-Q / 2))."""
    xy, co = np.asarray(xy, np.float64), np.asarray(co, np.float64)
    dx = xy[0] - np.arange(W, dtype=np.float64)[None, :]
    dy = xy[1] - np.arange(H, dtype=np.float64)[:, None]
    a, b, c, op = co
    Q = a * dx * dx + 2.0 * b * dx * dy + c * dy * dy
    tau = 2.0 * math.log(op / float(THRESH)) if op > 0 else -math.inf
    gamma = 2.0 ** -21 * (a * dx * dx + 2.0 * np.abs(b * dx * dy) + c * dy * dy) + 2.0 ** -22 * abs(tau)
    alpha = np.minimum(float(CAP), op * np.exp(-0.5 * Q))
    return Q, tau, gamma, alpha


def alpha_map_check(xy, co, radius, W, H, blended, alpha_img):
    """One frame's blend decisions (`blended`, bool H x W) and alphas (`alpha_img`) against fp64.
    -> dict: must_lost / must_gained  pixels outside the band |Q - tau| <= 2 gamma decided against
    fp64 (a conservative cull and a correct exponent leave both 0); lost / gained  the same inside
    the band (rounding flips); n64  pixels fp64 blends; in_band  of those, inside the band;
    alpha_excess  the largest |alpha - alpha64| / (alpha64 (exp(gamma / 2) - 1 + 2^-21)) over the
    blended pixels outside the band; worst_lost  the largest (tau - Q) / gamma of a lost pixel."""
    Q, tau, gamma, alpha = band(xy, co, W, H)
    rect = rect_mask(xy, radius, W, H) if radius > 0 else np.zeros((H, W), bool)
    want = rect & (Q <= tau)
    inb = np.abs(Q - tau) <= 2.0 * gamma
    lost_all, gained_all = want & ~blended, blended & ~want
    sure = blended & want & ~inb
    tol = alpha * (np.expm1(0.5 * gamma) + 2.0 ** -21)
    with np.errstate(divide="ignore", invalid="ignore"):
        excess = float((np.abs(alpha_img.astype(np.float64) - alpha)[sure] / tol[sure]).max()) if sure.any() else 0.0
        worst = float(((tau - Q) / gamma)[lost_all].max()) if lost_all.any() else 0.0
    return dict(must_lost=int((lost_all & ~inb).sum()), must_gained=int((gained_all & ~inb).sum()),
                lost=int((lost_all & inb).sum()), gained=int((gained_all & inb).sum()), n64=int(want.sum()),
                in_band=int((want & inb).sum()), alpha_excess=excess, worst_lost=worst)


def record(kind, case, **values):
    """One JSON line appended to $GSR_SHAPE_RECORD when set (profiles/r12_shape_margins.jsonl is made
    of these): the yardsticks the shape tests' bars are stated against."""
    import json
    import os
    path = os.environ.get("GSR_SHAPE_RECORD")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(json.dumps(dict(kind=kind, case=case, **values)) + "\n")


def recorded(kind):
    """{case: record} of one kind from profiles/r12_shape_margins.jsonl."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                        "r12_shape_margins.jsonl")
    out = {}
    with open(path) as f:
        for line in f:
            r = json.loads(line)
            if r["kind"] == kind:
                out[r["case"]] = r
    return out
