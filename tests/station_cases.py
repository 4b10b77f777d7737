"""Inputs of the station tests (test_station_cpu.py, test_gpu_station.py): a shell hierarchy around
the station, its cube-face cameras, cuts, and the single-view yardstick frame.

Every case is small: 60 000 leaves in the shell [1, 25] around the origin, 256 x 256 faces with
tanfov = 1.  The hierarchy and its cut are built once per process and never written to.
"""
from __future__ import annotations

import functools
import math

import numpy as np

LEAVES, FACE, TAU = 60_000, 256, 6.0
BG = (0.1, 0.2, 0.3)


@functools.lru_cache(maxsize=None)
def shell(device, skybox=0, leaves=LEAVES, seed=3):
    from gs_train.synthetic import synthetic_lod_hierarchy
    return synthetic_lod_hierarchy(leaves, FACE, FACE, device, seed=seed, skybox=skybox, zmin=1.0, zmax=25.0,
                                   log_scale_mean=-3.5, layout="shell")


def faces(n_faces, center=(0.0, 0.0, 0.0), rig=None, W=FACE):
    from gs_train.synthetic import cube_face_cameras
    return cube_face_cameras(W, n_faces, center, rig=rig)


def mild_rig():
    """posed_cases' "mild" pose as a station: its world-to-camera rotation as the rig's, its camera
    centre as the station's."""
    import posed_cases as PC
    p = PC.pose("mild", FACE, FACE)
    view = p["view"].astype(np.float64).reshape(4, 4)
    return view[:3, :3].T.copy(), p["campos"].astype(np.float32)


@functools.lru_cache(maxsize=None)
def cut(device, skybox=0, tau=TAU, center=(0.0, 0.0, 0.0), leaves=LEAVES):
    """(ri, pi, w) of the shell hierarchy at `center`, the skybox rows appended with weight 1 and
    themselves as parent (render_post's rows), made with expand_to_size / get_interpolation_weights
    directly -- not through StationRenderer."""
    import torch
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    from gs_train.synthetic import tau_threshold
    h = shell(device, skybox, leaves)
    Nn = h["nodes"].shape[0]
    N = h["means3D"].shape[0]
    ri, pi, ni = (torch.zeros(Nn, dtype=torch.int32, device=device) for _ in range(3))
    w = torch.zeros(Nn, device=device)
    k = torch.zeros(Nn, dtype=torch.int32, device=device)
    thr = float(np.float32(tau_threshold(tau, 1.0, FACE)))
    vp = torch.tensor(np.asarray(center, np.float32), device=device)
    n = expand_to_size(h["nodes"], h["boxes"], thr, vp, torch.zeros(3), ri, pi, ni)
    get_interpolation_weights(ni[:n], thr, h["nodes"], h["boxes"], vp.cpu(), torch.zeros(3), w, k)
    sky = torch.arange(N - skybox, N, dtype=torch.int32, device=device)
    return (torch.cat([ri[:n], sky]).contiguous(), torch.cat([pi[:n], sky]).contiguous(),
            torch.cat([w[:n], torch.ones(skybox, device=device)]).contiguous())


def single_view(h, cam, ri, pi, w, device, bg=BG, sh_degree=3):
    """The yardstick: the fused single-view cut frame of one face (K, colour, inverse depth, radii),
    held to the oracle by test_gpu_lod.py."""
    import torch
    from diff_gaussian_rasterization import _C
    t = lambda x: torch.tensor(np.asarray(x), dtype=torch.float32, device=device)
    e = torch.empty(0, device=device)
    kids = torch.zeros(ri.shape[0], dtype=torch.int32, device=device)
    with torch.no_grad():
        out = _C.rasterize_gaussians(t(bg), h["means3D"], e, h["opacities"], h["scales"], h["rotations"], 1.0, e,
                                     t(cam["view"]).reshape(4, 4), t(cam["proj"]).reshape(4, 4), float(cam["tanfovx"]),
                                     float(cam["tanfovy"]), int(cam["H"]), int(cam["W"]), h["shs"], int(sh_degree),
                                     t(cam["campos"]), False, False, ri, pi, w, kids, True, need_backward=False)
    return out[0], out[1], out[2], out[3]


def near_plane_leaves(device):
    """A hand-made model for face 0 of an unrotated station at the origin (its view matrix is the
    identity, so a mean's view depth is its z, exactly): three leaves on the optical axis at the
    float32 below 0.2, at 0.2 and at the float32 above it, then 61 leaves well in front.  Returns
    (tensors, sides): sides[i] = True when leaf i's view depth, computed here on the host in float32
    by the rasterizer's expression, is > 0.2 (kept by the near test)."""
    import torch
    rng = np.random.default_rng(17)
    lim = np.float32(0.2)
    z3 = np.array([np.nextafter(lim, np.float32(0)), lim, np.nextafter(lim, np.float32(1))], np.float32)
    n = 64
    means = np.zeros((n, 3), np.float32)
    means[:3, 2] = z3
    means[3:, 2] = rng.uniform(2.0, 6.0, n - 3)
    means[3:, :2] = rng.uniform(-0.6, 0.6, (n - 3, 2)) * means[3:, 2:3]
    view = faces(4)[0]["view"].reshape(4, 4)  # row-major W2C^T, read column-major by the kernels: m[k] = view.flat[k]
    m = view.reshape(-1)
    depth = (m[2] * means[:, 0] + m[6] * means[:, 1]).astype(np.float32)
    depth = (depth + m[10] * means[:, 2]).astype(np.float32)
    depth = (depth + m[14]).astype(np.float32)
    sides = depth > lim
    assert sides[:3].tolist() == [False, False, True] and bool(sides[3:].all())
    assert depth[0] < lim and depth[1] == lim and depth[2] > lim
    scales = np.full((n, 3), 0.01, np.float32)
    scales[3:] = 0.05
    rots = np.zeros((n, 4), np.float32)
    rots[:, 0] = 1.0
    shs = np.zeros((n, 16, 3), np.float32)
    shs[:, 0, :] = rng.normal(0.5, 0.5, (n, 3))
    shs[:, 1:, :] = rng.normal(0, 0.05, (n, 15, 3))
    t = lambda a: torch.tensor(a, device=device)
    tensors = dict(means3D=t(means), scales=t(scales), rotations=t(rots),
                   opacities=t(rng.uniform(0.3, 0.9, (n, 1)).astype(np.float32)), shs=t(shs))
    return tensors, sides


def reference_station_key(centers, decimals=2):
    """render_position.py:24-31's grouping, restated: cameras keyed by np.round(center, 2), groups in
    the dict's insertion order."""
    grouped = {}
    for i, c in enumerate(centers):
        key = tuple(np.round(np.asarray(c), decimals=decimals))
        grouped.setdefault(key, []).append(i)
    return list(grouped.values())


def yaw(deg):
    a = math.radians(deg)
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
