"""The model from a point cloud (include/gsr_model_init.h, csrc/model_init.hip): the front of
scripts/full_train.py that turns a LiDAR / COLMAP cloud into Gaussians.

create_from_cloud restates GaussianModel.create_from_pcd (scene/gaussian_model.py:163-278):

  without a scaffold   [skybox | cloud] rows: the skybox on a sphere of 10 x the cloud's radius,
                       kNN scales over all rows, opacity 0.02 (skybox rows the raw value 0.7)
  with a scaffold      the chunk's cloud rows (kNN over them alone, opacity 0.01) behind the rows of
                       the coarse scaffold inside the ring around the chunk and the scaffold's skybox
                       (gs_train.scaffold.load_scaffold; bounds = the chunk's center.txt / extent.txt
                       values), SH padded with zeros

The two uniform draws behind the skybox come from torch.rand in the reference's order, so a seeded
run consumes the generator as the reference does.  There is no CPU path."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._native import check, lib, ptr, require_gpu, stream
from .harness import GaussianSet

PLAIN, SKYBOX = 0, 1  # GSR_MODEL_INIT_PLAIN, GSR_MODEL_INIT_SKYBOX


def _rows(name, t, width):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    require_gpu(t)
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: expected float32")
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError(f"{name}: expected shape (N, {width}), got {tuple(t.shape)}")
    return t.detach().contiguous()


def init_cloud(points, colors, u_theta=None, u_phi=None, M=16):
    """gsr_model_init_cloud.  points, colors: (N, 3) float32 on the device, N >= 1; u_theta, u_phi:
    (S,) uniform draws for S skybox rows (both None: plain mode).  Returns the raw arrays
    (xyz, features (S+N, M, 3), opacity_raw, scaling_raw, rotation) and (mean (3,), radius) as
    numpy float32."""
    pts = _rows("points", points, 3)
    col = _rows("colors", colors, 3)
    if col.shape[0] != pts.shape[0] or col.device != pts.device:
        raise ValueError("colors: one row per point, on the points' device")
    N = pts.shape[0]
    if N < 1:
        raise ValueError("points: the cloud is empty")
    if (u_theta is None) != (u_phi is None):
        raise ValueError("u_theta and u_phi come together")
    S = 0
    if u_theta is not None:
        for name, u in (("u_theta", u_theta), ("u_phi", u_phi)):
            require_gpu(u)
            if u.dtype != torch.float32 or u.dim() != 1 or u.device != pts.device:
                raise ValueError(f"{name}: expected (S,) float32 on the points' device")
        if u_theta.shape != u_phi.shape or u_theta.shape[0] < 1:
            raise ValueError("u_theta, u_phi: expected the same length S >= 1")
        S = u_theta.shape[0]
        u_theta, u_phi = u_theta.detach().contiguous(), u_phi.detach().contiguous()
    if not 1 <= int(M) <= 16:
        raise ValueError("M: 1 to 16 SH coefficients")
    dev = pts.device
    P = S + N
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    xyz, feat, op, sc, rot = new(P, 3), new(P, int(M), 3), new(P, 1), new(P, 3), new(P, 4)
    L = lib()
    scratch = torch.empty(L.gsr_model_init_scratch_bytes(N, S), dtype=torch.uint8, device=dev)
    bounds = (ctypes.c_float * 4)()
    with torch.cuda.device(dev):
        check(L.gsr_model_init_cloud(N, ptr(pts), ptr(col), S, ptr(u_theta), ptr(u_phi), int(M),
                                     SKYBOX if S else PLAIN, ptr(xyz), ptr(feat), ptr(op), ptr(sc), ptr(rot), bounds,
                                     ptr(scratch), stream(dev)), "gsr_model_init_cloud")
    b = np.array(list(bounds), dtype=np.float32)
    return (xyz, feat, op, sc, rot), (b[:3], b[3])


def scaffold_merge(scaffold, center, extent, chunk):
    """gsr_scaffold_merge_count + _write: the scaffold rows selected for a chunk with `center` and
    `extent` (3 floats each) in front of `chunk` = (xyz, features (Pc, M, 3), opacity_raw, scaling_raw,
    rotation).  scaffold: an object with xyz, shs (Ps, 4, 3), opacity_raw, log_scales, rotations and
    skybox_points (gs_train.scaffold.Scaffold).  Returns the five merged arrays and K."""
    s_arr = [_rows("scaffold.xyz", scaffold.xyz, 3), None, _rows("scaffold.opacity_raw", scaffold.opacity_raw, 1),
             _rows("scaffold.log_scales", scaffold.log_scales, 3), _rows("scaffold.rotations", scaffold.rotations, 4)]
    Ps = s_arr[0].shape[0]
    shs = scaffold.shs
    require_gpu(shs)
    if shs.dtype != torch.float32 or tuple(shs.shape) != (Ps, 4, 3):
        raise ValueError(f"scaffold.shs: expected ({Ps}, 4, 3) float32, got {tuple(shs.shape)}")
    s_arr[1] = shs.detach().contiguous()
    c_xyz, c_feat, c_op, c_sc, c_rot = chunk
    c_arr = [_rows("chunk xyz", c_xyz, 3), None, _rows("chunk opacity", c_op, 1), _rows("chunk scaling", c_sc, 3),
             _rows("chunk rotation", c_rot, 4)]
    Pc = c_arr[0].shape[0]
    require_gpu(c_feat)
    if c_feat.dtype != torch.float32 or c_feat.dim() != 3 or c_feat.shape[0] != Pc or c_feat.shape[2] != 3 \
            or not 4 <= c_feat.shape[1] <= 16:
        raise ValueError(f"chunk features: expected ({Pc}, M, 3) float32 with 4 <= M <= 16")
    c_arr[1] = c_feat.detach().contiguous()
    M = c_feat.shape[1]
    dev = s_arr[0].device
    for a, n in ((s_arr, Ps), (c_arr, Pc)):
        if any(t.shape[0] != n or t.device != dev for t in a):
            raise ValueError("scaffold_merge: one row per Gaussian in every array, all on one device")
    S = int(scaffold.skybox_points)
    if S < 0:
        raise ValueError("scaffold.skybox_points: expected >= 0")
    c3 = (ctypes.c_float * 3)(*[float(v) for v in center])
    e3 = (ctypes.c_float * 3)(*[float(v) for v in extent])
    L = lib()
    scratch = torch.empty(L.gsr_scaffold_merge_scratch_bytes(Ps), dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(L.gsr_scaffold_merge_count(Ps, S, ptr(s_arr[0]), c3, e3, ptr(scratch), ptr(count), stream(dev)),
              "gsr_scaffold_merge_count")
        K = int(count.item())  # the one host read: the output's size
        P = K + Pc
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        out = (new(P, 3), new(P, M, 3), new(P, 1), new(P, 3), new(P, 4))
        check(L.gsr_scaffold_merge_write(Ps, K, *[ptr(t) for t in s_arr], Pc, M, *[ptr(t) for t in c_arr],
                                         *[ptr(t) for t in out], ptr(scratch), stream(dev)),
              "gsr_scaffold_merge_write")
    return out, K


def gaussians_from_raw(xyz, features, opacity_raw, scaling_raw, rotation, n_images, sh_degree=0,
                       spatial_lr_scale=1.0) -> GaussianSet:
    """A joined-layout GaussianSet around raw parameter arrays, as they are (GaussianSet's
    constructor takes activated values and re-derives the raw ones through log and logit)."""
    g = object.__new__(GaussianSet)
    dev = xyz.device
    P = xyz.shape[0]
    g.joined = True
    g._xyz = torch.nn.Parameter(xyz)
    g._features = torch.nn.Parameter(features)
    g._opacity = torch.nn.Parameter(opacity_raw)
    g._scaling = torch.nn.Parameter(scaling_raw)
    g._rotation = torch.nn.Parameter(rotation)
    g._exposure = torch.nn.Parameter(torch.eye(3, 4, device=dev)[None].repeat(int(n_images), 1, 1))
    g.active_sh_degree = int(sh_degree)
    g.spatial_lr_scale = spatial_lr_scale
    g.max_radii2D = torch.zeros(P, device=dev)
    g.xyz_gradient_accum = torch.zeros((P, 1), device=dev)
    g.denom = torch.zeros((P, 1), device=dev)
    return g


def create_from_cloud(points, colors, n_images, spatial_lr_scale, skybox_points=0, scaffold=None, bounds=None,
                      sh_degree=3, generator=None):
    """create_from_pcd(pcd, cam_infos, spatial_lr_scale, skybox_points, scaffold_file, bounds_file).

    points, colors: (N, 3) float32 on the device.  scaffold: a gs_train.scaffold.Scaffold (the loaded
    scaffold_file) with bounds = (center, extent), 3 floats each (bounds_file's center.txt and
    extent.txt); a non-zero skybox_points is then overridden to 0 (:183-185).  sh_degree: the model's
    max_sh_degree (1 for the coarse model).  generator: the device generator the skybox draws come
    from (default: the device's own, as the reference).
    Returns (GaussianSet in the joined layout with active degree 0, skybox_points, scaffold_points);
    scaffold_points is None without a scaffold."""
    if (scaffold is None) != (bounds is None):
        raise ValueError("scaffold and bounds come together (scaffold_file and bounds_file)")
    S = int(skybox_points)
    if S < 0:
        raise ValueError("skybox_points: expected >= 0")
    pts = _rows("points", points, 3)
    if scaffold is not None:
        S = 0
    M = (int(sh_degree) + 1) ** 2
    if not 0 <= int(sh_degree) <= 3:
        raise ValueError("sh_degree: 0 to 3")
    u_theta = u_phi = None
    if S > 0:
        u_theta = torch.rand(S, device=pts.device, generator=generator)
        u_phi = torch.rand(S, device=pts.device, generator=generator)
    arrays, _ = init_cloud(pts, colors, u_theta, u_phi, M)
    scaffold_points = None
    if scaffold is not None:
        if M < 4:
            raise ValueError("a scaffold carries degree-1 SH: sh_degree >= 1")
        center, extent = bounds
        if len(center) != 3 or len(extent) != 3:
            raise ValueError("bounds: (center, extent), 3 floats each")
        arrays, scaffold_points = scaffold_merge(scaffold, center, extent, arrays)
        S = int(scaffold.skybox_points)
    g = gaussians_from_raw(*arrays, n_images=n_images, sh_degree=0, spatial_lr_scale=spatial_lr_scale)
    return g, S, scaffold_points
