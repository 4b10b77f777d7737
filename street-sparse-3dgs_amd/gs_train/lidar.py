"""A chunk's LiDAR cloud on the device (include/gsr_lidar.h, csrc/lidar.hip).

prepare_chunk_cloud replaces process_lidar_points of the reference's chunker
(preprocess/ss_make_chunk.py:36-305) from the decoded survey points on: the crop to the chunk's box,
the filter "within max_distance of the reconstructed mesh" (an Open3D raycasting scene on the host
there) and the voxel mean that makes the LiDAR initial points (Open3D's voxel_down_sample).  Its two
products are what the rest of this package takes: ChunkCloud.save_ply writes the chunk.ply that
GtPointCloud.from_ply reads, and init_points / init_colors_u8 are create_from_cloud's cloud.  LAZ
decoding and the tile selection (:237-270) stay with the caller.

The rule is stated in gsr_lidar.h: strict fp32 crop on x and y, Euclidean distance to the closest
point of any closed triangle <= max_distance, fp64 voxel means in ascending (iz, iy, ix) order."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ._native import check, lib, ptr, require_gpu, stream
from .gtcloud import read_ply_vertex_columns, read_ply_vertex_header


def read_ply_mesh(path):
    """(vertices (V, 3) float32, faces (F, 3) int32) of a triangle mesh PLY: `format ascii 1.0` or
    `format binary_little_endian 1.0`, a vertex element with float or double x, y, z (other scalar
    properties allowed) and a face element whose only property is `list uchar int|uint vertex_indices`
    (or vertex_index), every face a triangle.  Elements between the two must be scalar-only.  Raises
    ValueError on anything else."""
    header = read_ply_vertex_header(path)
    body, fmt, elements, vi, count, props = header
    types = dict(props)
    for c in "xyz":
        if types.get(c) not in ("f4", "f8"):
            raise ValueError(f"{path}: vertex property {c!r} is missing or not float or double")
    vertices = np.ascontiguousarray(np.stack(read_ply_vertex_columns(path, header, "xyz"), 1).astype(np.float32))
    names = [e[0] for e in elements]
    if "face" not in names or names.index("face") < vi:
        raise ValueError(f"{path}: no face element after the vertex element")
    fi = names.index("face")
    fname, F, fprops, flists = elements[fi]
    if len(fprops) != 1 or fprops[0][0] not in ("vertex_indices", "vertex_index") or fprops[0][1] is not None:
        raise ValueError(f"{path}: the face element must have the one property `list uchar int vertex_indices`")
    ctype, itype = flists[fprops[0][0]]
    if ctype != "u1" or itype not in ("i4", "u4"):
        raise ValueError(f"{path}: face property must be `list uchar int|uint vertex_indices`, got list {ctype} {itype}")
    for e in elements[vi + 1:fi]:
        if any(t is None for _, t in e[2]):
            raise ValueError(f"{path}: list property in element {e[0]!r} between the vertices and the faces")
    if fmt[0] == "ascii":
        tok = body.split()
        skip = sum(e[1] * len(e[2]) for e in elements[:fi])
        if len(tok) < skip + 4 * F:
            raise ValueError(f"{path}: truncated face data")
        try:
            rows = np.array(tok[skip:skip + 4 * F], dtype=np.int64).reshape(F, 4)
        except ValueError as e:
            raise ValueError(f"{path}: malformed ascii face data (triangles only)") from e
        n, idx = rows[:, 0], rows[:, 1:]
    else:
        off = sum(e[1] * np.dtype([(n, "<" + t) for n, t in e[2]]).itemsize for e in elements[:fi] if e[2])
        dt = np.dtype([("n", "u1"), ("v", "<" + itype, (3,))])
        if len(body) < off + F * dt.itemsize:
            raise ValueError(f"{path}: truncated face data (triangles only)")
        rows = np.frombuffer(body, dtype=dt, count=F, offset=off)
        n, idx = rows["n"], rows["v"].astype(np.int64)
    if F and not bool((n == 3).all()):
        raise ValueError(f"{path}: a face is not a triangle")
    if F and (idx.min() < 0 or idx.max() >= count):
        raise ValueError(f"{path}: a face index is out of range")
    return vertices, np.ascontiguousarray(idx.astype(np.int32))


def _device_rows(name, a, device, dtype=torch.float32):
    if isinstance(a, torch.Tensor):
        require_gpu(a)
        t = a.detach()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(device)
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype != dtype:
        raise ValueError(f"{name}: expected shape (N, 3) {dtype}, got {tuple(t.shape)} {t.dtype}")
    return t.contiguous()


def crop_bounds(center, extent) -> np.ndarray:
    """The crop's fp32 bounds x_lo, x_hi, y_lo, y_hi: c -+ e/2 with c, e and both operations in fp32."""
    c = np.asarray(center, dtype=np.float32)
    e = np.asarray(extent, dtype=np.float32)
    if c.shape[0] < 2 or e.shape[0] < 2:
        raise ValueError("center, extent: at least x and y")
    half = e[:2] / np.float32(2)
    return np.array([c[0] - half[0], c[0] + half[0], c[1] - half[1], c[1] + half[1]], dtype=np.float32)


def _near_mask(points, index, max_distance, box):
    P = points.shape[0]
    out = torch.empty(P, dtype=torch.uint8, device=points.device)
    b = None
    if box is not None:
        b = (ctypes.c_float * 4)(*[float(v) for v in np.asarray(box, dtype=np.float32)])
    with torch.cuda.device(points.device):
        check(lib().gsr_mesh_near_mask(P, ptr(points), index, float(max_distance), b, ptr(out),
                                       stream(points.device)), "gsr_mesh_near_mask")
    return out.bool()


class MeshIndex:
    """vertices: (V, 3) float32, finite; faces: (F, 3) int32 into them (tensors or arrays); max_distance:
    the distance the index is built for (queries at another one stay exact).  Owns the device index: a
    uniform grid of the occupied cells with every triangle listed, as its three vertices, in each cell
    it can be within reach of, and an oversize list for triangles that would cover too many cells."""

    def __init__(self, vertices, faces, max_distance: float = 0.1, device="cuda"):
        self._index = None
        for a in (vertices, faces):
            if isinstance(a, torch.Tensor):
                require_gpu(a)
        dev = vertices.device if isinstance(vertices, torch.Tensor) else torch.device(device)
        v = _device_rows("vertices", vertices, dev)
        f = _device_rows("faces", faces, dev, torch.int32)
        if v.shape[0] < 1 or f.shape[0] < 1:
            raise ValueError("a mesh needs at least one vertex and one triangle")
        self.max_distance = float(max_distance)
        if not (self.max_distance > 0.0 and np.isfinite(self.max_distance)):
            raise ValueError("max_distance: expected a finite value > 0")
        self.device = v.device
        with torch.cuda.device(self.device):
            h = lib().gsr_mesh_index_create(v.shape[0], ptr(v), f.shape[0], ptr(f), self.max_distance,
                                            stream(self.device))
        if not h:
            from diff_gaussian_rasterization._lib import last_error
            raise RuntimeError(f"gsr_mesh_index_create failed: {last_error()}")
        self._index = ctypes.c_void_p(h)

    @classmethod
    def from_ply(cls, path, max_distance: float = 0.1, device="cuda"):
        return cls(*read_ply_mesh(path), max_distance=max_distance, device=device)

    @property
    def handle(self):
        if self._index is None:
            raise RuntimeError("the mesh index has been released")
        return self._index

    def close(self) -> None:
        ix, self._index = self._index, None
        if ix is not None and ix.value:
            lib().gsr_mesh_index_destroy(ix)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def info(self) -> dict:
        v = (ctypes.c_int64 * 9)()
        check(lib().gsr_mesh_index_info(self.handle, v, 9), "gsr_mesh_index_info")
        return {"vertices": int(v[0]), "triangles": int(v[1]), "cells": int(v[2]), "references": int(v[3]),
                "oversize": int(v[4]), "bytes": int(v[5]), "grid": (int(v[6]), int(v[7]), int(v[8]))}

    def near_mask(self, points: torch.Tensor, box=None, max_distance: Optional[float] = None) -> torch.Tensor:
        """(P,) bool: the point is finite, inside `box` (crop_bounds' x_lo, x_hi, y_lo, y_hi; None: no
        crop) and within max_distance (default: the index's own) of the mesh."""
        require_gpu(points)
        if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
            raise ValueError("points: expected (P, 3) float32")
        if points.device != self.device:
            raise ValueError("points: not on the mesh's device")
        d = self.max_distance if max_distance is None else float(max_distance)
        return _near_mask(points.detach().contiguous(), self.handle, d, box)


def voxel_downsample(points, colors, voxel_size: float):
    """Open3D's voxel_down_sample: (points (M, 3) float32, colors (M, 3) float32 or None, counts (M,)
    int32), one row per occupied voxel in ascending (iz, iy, ix) order, the fp64 means rounded to fp32.
    points: (P, 3) float32 on the device, finite; colors: the same shape, or None."""
    return _voxel_mean(points, colors, None, voxel_size)


def _voxel_mean(points, colors, keep, voxel_size):
    require_gpu(points, colors, keep)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("points: expected (P, 3) float32")
    if colors is not None and (colors.shape != points.shape or colors.dtype != torch.float32):
        raise ValueError("colors: expected the shape and type of points")
    voxel_size = float(voxel_size)
    if not (voxel_size > 0.0 and np.isfinite(voxel_size)):
        raise ValueError("voxel_size: expected a finite value > 0")
    points = points.detach().contiguous()
    colors = colors.detach().contiguous() if colors is not None else None
    P, dev = points.shape[0], points.device
    L = lib()
    scratch = torch.empty(L.gsr_voxel_mean_scratch_bytes(P), dtype=torch.uint8, device=dev)
    out_xyz = torch.empty((P, 3), dtype=torch.float32, device=dev)
    out_col = torch.empty((P, 3), dtype=torch.float32, device=dev) if colors is not None else None
    out_cnt = torch.empty(P, dtype=torch.int32, device=dev)
    n = ctypes.c_int64(0)
    with torch.cuda.device(dev):
        check(L.gsr_voxel_mean(P, ptr(points), ptr(colors), ptr(keep), voxel_size, ptr(scratch), ptr(out_xyz),
                               ptr(out_col), ptr(out_cnt), ctypes.byref(n), stream(dev)), "gsr_voxel_mean")
    m = int(n.value)
    return out_xyz[:m].clone(), (out_col[:m].clone() if out_col is not None else None), out_cnt[:m].clone()


@dataclass
class ChunkCloud:
    """points / colors: the cropped and mesh-filtered cloud (what chunk.ply holds); init_points /
    init_colors_u8: its voxel mean, the LiDAR initial points (None with lidar_init=False)."""
    points: torch.Tensor
    colors: Optional[torch.Tensor]
    init_points: Optional[torch.Tensor]
    init_colors_u8: Optional[torch.Tensor]

    def save_ply(self, path) -> None:
        """chunk.ply: binary little-endian, float32 x, y, z (and uchar red, green, blue when the cloud
        has colours), as the reference leaves it after its float conversion (:296-301)."""
        xyz = self.points.detach().cpu().numpy().astype("<f4")
        fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
        lines = ["ply", "format binary_little_endian 1.0", f"element vertex {len(xyz)}",
                 "property float x", "property float y", "property float z"]
        if self.colors is not None:
            fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
            lines += ["property uchar red", "property uchar green", "property uchar blue"]
        rows = np.zeros(len(xyz), np.dtype(fields))
        rows["x"], rows["y"], rows["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        if self.colors is not None:
            c = (self.colors.detach().cpu().numpy().astype(np.float64) * 255).clip(0, 255).astype(np.uint8)
            rows["red"], rows["green"], rows["blue"] = c[:, 0], c[:, 1], c[:, 2]
        with open(path, "wb") as f:
            f.write(("\n".join(lines) + "\nend_header\n").encode("ascii"))
            f.write(rows.tobytes())


def prepare_chunk_cloud(points, colors, center, extent, mesh: Optional[MeshIndex] = None, max_distance: float = 0.1,
                        density: float = 2000, lidar_init: bool = True) -> ChunkCloud:
    """process_lidar_points from the decoded points on.  points: (P, 3) float32 on the device, in the
    chunk's (translated) frame; colors: (P, 3) float32 in [0, 1], or None; center, extent: the chunk's
    center.txt and extent.txt (x and y are used); mesh: the reconstructed mesh's MeshIndex, None skips
    the distance filter (the reference does when the mesh has no triangles, :174-176); density: the
    most initial points per cubic metre (LiDAR_downsample_density).  Points with a NaN or Inf
    coordinate are dropped in either case."""
    require_gpu(points, colors)
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
        raise ValueError("points: expected (P, 3) float32")
    if colors is not None and (colors.shape != points.shape or colors.dtype != torch.float32):
        raise ValueError("colors: expected the shape and type of points")
    if mesh is not None and mesh.device != points.device:
        raise ValueError("points: not on the mesh's device")
    points = points.detach().contiguous()
    box = crop_bounds(center, extent)
    keep = _near_mask(points, mesh.handle if mesh is not None else None, max_distance, box)
    kept = points[keep]
    kept_colors = colors.detach()[keep] if colors is not None else None
    init_points = init_u8 = None
    if lidar_init:
        if not density > 0:
            raise ValueError("density: expected > 0")
        voxel_size = (1.0 / density) ** (1 / 3)  # :73
        init_points, init_colors, _ = _voxel_mean(kept, kept_colors, None, voxel_size)
        if init_colors is not None:
            init_u8 = (init_colors.double() * 255).to(torch.uint8)  # :287: truncated
        else:
            init_u8 = torch.zeros((init_points.shape[0], 3), dtype=torch.uint8, device=points.device)  # :289
    return ChunkCloud(kept, kept_colors, init_points, init_u8)
