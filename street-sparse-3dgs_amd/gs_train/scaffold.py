"""The files between the coarse stage and the chunks: a scaffold directory holds point_cloud.ply
(GaussianModel.save_ply, scene/gaussian_model.py:459-471,509-527) and pc_info.txt, the skybox count
as Scene.save writes it (scene/__init__.py:101-102).

save_scaffold writes them from a trained coarse model; load_scaffold reads them back as
create_from_pcd does (load_ply_file, :308-341, by property name) for
gs_train.model_init.create_from_cloud(scaffold=...) and Hierarchy.to_model(skybox_rows=...).
The PLY header parser is gs_train.gtcloud's; plyfile is not needed."""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np
import torch

from .gtcloud import read_ply_vertex_columns, read_ply_vertex_header

PLY_NAME = "point_cloud.ply"
INFO_NAME = "pc_info.txt"


def ply_attributes(M: int) -> list:
    """construct_list_of_attributes for M SH coefficients per row."""
    return (["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)]
            + [f"f_rest_{i}" for i in range(3 * (M - 1))] + ["opacity"] + [f"scale_{i}" for i in range(3)]
            + [f"rot_{i}" for i in range(4)])


@torch.no_grad()
def save_scaffold(dir, gaussians, skybox_points: int) -> None:
    """dir/point_cloud.ply (binary_little_endian 1.0, one vertex element, every property float, the
    raw parameters as they are) and dir/pc_info.txt.  The rows are packed by one torch.cat on the
    model's device and copied to the host once."""
    g = gaussians
    f = g.get_features.detach()
    P, M = f.shape[0], f.shape[1]
    rows = torch.cat([g._xyz.detach(), torch.zeros_like(g._xyz), f[:, 0, :],
                      f[:, 1:, :].transpose(1, 2).reshape(P, 3 * (M - 1)),  # channel-major (:515)
                      g._opacity.detach().reshape(P, 1), g._scaling.detach(), g._rotation.detach()], dim=1)
    names = ply_attributes(M)
    assert rows.shape[1] == len(names) and rows.dtype == torch.float32
    host = rows.contiguous().cpu().numpy().astype("<f4", copy=False)
    os.makedirs(dir, exist_ok=True)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % P
    header += "".join(f"property float {n}\n" for n in names) + "end_header\n"
    with open(os.path.join(dir, PLY_NAME), "wb") as out:
        out.write(header.encode("ascii"))
        out.write(host.tobytes())
    with open(os.path.join(dir, INFO_NAME), "w") as out:
        out.write(str(int(skybox_points)))


@dataclass
class Scaffold:
    """A loaded scaffold: raw parameters, float32.  shs: (Ps, 4, 3), coefficient-major as the model
    keeps them."""
    xyz: torch.Tensor
    shs: torch.Tensor
    opacity_raw: torch.Tensor
    log_scales: torch.Tensor
    rotations: torch.Tensor
    skybox_points: int

    def skybox_rows(self):
        """(xyz, log_scales, rotations, opacities, shs) of the skybox rows for
        Hierarchy.to_model(skybox_rows=...): activated opacities, as create_from_hier takes them
        (scene/gaussian_model.py:393)."""
        S = self.skybox_points
        return (self.xyz[:S], self.log_scales[:S], self.rotations[:S], torch.sigmoid(self.opacity_raw[:S]),
                self.shs[:S])


def _numbered(names, prefix):
    return sorted((n for n in names if n.startswith(prefix)), key=lambda n: int(n.split("_")[-1]))


def load_scaffold(dir, device="cuda") -> Scaffold:
    """dir/point_cloud.ply and dir/pc_info.txt, as create_from_pcd reads a scaffold_file (:226-235):
    properties by name, f_rest_*, scale_* and rot_* in the order of their numeric suffix, whatever
    their order in the file; float / float32 (or double) properties, ascii or binary little-endian.
    Raises ValueError naming the file on a truncated file, a missing property or an SH degree other
    than the coarse model's 1 (load_ply_file(path, 1), :226)."""
    path = os.path.join(dir, PLY_NAME)
    header = read_ply_vertex_header(path)
    props = header[5]
    names = [n for n, _ in props]
    rest, scale, rot = _numbered(names, "f_rest_"), _numbered(names, "scale_"), _numbered(names, "rot")
    M = 4
    want = ["x", "y", "z", "opacity", "f_dc_0", "f_dc_1", "f_dc_2"]
    for n in want:
        if n not in names:
            raise ValueError(f"{path}: the vertex element has no property {n!r}")
    if len(rest) != 3 * M - 3:
        raise ValueError(f"{path}: {len(rest)} f_rest_* properties, expected {3 * M - 3} (SH degree 1)")
    if len(scale) != 3 or len(rot) != 4:
        raise ValueError(f"{path}: expected 3 scale_* and 4 rot_* properties, got {len(scale)} and {len(rot)}")
    order = want + rest + scale + rot
    types = dict(props)
    for n in order:
        if types[n] not in ("f4", "f8"):
            raise ValueError(f"{path}: vertex property {n!r} is not float or double")
    cols = read_ply_vertex_columns(path, header, order)
    a = np.stack([np.asarray(c, dtype=np.float32) for c in cols], 1)
    P = a.shape[0]
    shs = np.concatenate([a[:, 4:7].reshape(P, 1, 3),
                          a[:, 7:7 + 3 * (M - 1)].reshape(P, 3, M - 1).transpose(0, 2, 1)], 1)
    k = 7 + 3 * (M - 1)
    info = os.path.join(dir, INFO_NAME)
    with open(info) as f:
        line = f.readline()
    try:
        skybox = int(line)
    except ValueError as e:
        raise ValueError(f"{info}: expected the skybox count, got {line!r}") from e
    if not 0 <= skybox <= P:
        raise ValueError(f"{info}: skybox count {skybox} outside the file's {P} rows")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)
    return Scaffold(t(a[:, 0:3]), t(shs), t(a[:, 3:4]), t(a[:, k:k + 3]), t(a[:, k + 3:k + 7]), skybox)
