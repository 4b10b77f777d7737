"""The ground-truth point cloud constraint of densification (include/gsr_gtcloud.h, csrc/gtcloud.hip).

GtPointCloud replaces GaussianModel.load_gt_point_cloud + compare_points_to_gt
(scene/gaussian_model.py:796-962): the reference keeps the LiDAR cloud in a FAISS flat index and, on
every densification, copies the Gaussian positions to the host and scans every cloud point per
Gaussian.  Here the cloud is indexed once on the device (a uniform grid, 16 B per point + 12 B per
occupied cell) and the query is one kernel; gs_train.densify.densify_and_prune(..., gt_cloud=...)
runs it inside its plan.

The decision is defined in fp32, bit for bit (gsr_gtcloud.h): inside the cloud's XY bounds
(inclusive, no z test) and every cloud point with (dx*dx + dy*dy) + dz*dz > threshold**2."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._native import check, lib, ptr, require_gpu, stream

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
              "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
              "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_vertex_header(path):
    """The header of a PLY file up to its vertex element: (body bytes, format, elements, index of the
    vertex element, its row count, its [(property name, numpy type)]).  An element is [name, count,
    [(property name, numpy type or None for a list)], {list property name: (count type, item type)}].
    Reads `format ascii 1.0` and `format binary_little_endian 1.0`; raises ValueError on anything else
    (big-endian data, no vertex element, list properties in or before the vertex element)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    nl = data.find(b"\n", end)
    if nl < 0:
        raise ValueError(f"{path}: truncated PLY header")
    body = data[nl + 1:]
    fmt = None
    elements = []  # [name, count, [(property name, numpy type or None for a list)], {list name: types}]
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = tuple(w[1:])
        elif w[0] == "element" and len(w) == 3:
            elements.append([w[1], int(w[2]), [], {}])
        elif w[0] == "property" and elements:
            if w[1] == "list":
                if len(w) != 5 or w[2] not in _PLY_TYPES or w[3] not in _PLY_TYPES:
                    raise ValueError(f"{path}: unsupported PLY property line {line!r}")
                elements[-1][2].append((w[4], None))
                elements[-1][3][w[4]] = (_PLY_TYPES[w[2]], _PLY_TYPES[w[3]])
            elif len(w) == 3 and w[1] in _PLY_TYPES:
                elements[-1][2].append((w[2], _PLY_TYPES[w[1]]))
            else:
                raise ValueError(f"{path}: unsupported PLY property line {line!r}")
        else:
            raise ValueError(f"{path}: unsupported PLY header line {line!r}")
    if fmt not in (("ascii", "1.0"), ("binary_little_endian", "1.0")):
        raise ValueError(f"{path}: unsupported PLY format {' '.join(fmt or ())!r} (ascii or binary_little_endian 1.0)")
    names = [e[0] for e in elements]
    if "vertex" not in names:
        raise ValueError(f"{path}: no vertex element")
    vi = names.index("vertex")
    for e in elements[:vi + 1]:
        if any(t is None for _, t in e[2]):
            raise ValueError(f"{path}: list property in or before the vertex element")
    count, props = elements[vi][1:3]
    return body, fmt, elements, vi, count, props


def read_ply_vertex_columns(path, header, names):
    """The vertex element's properties `names` as a list of (count,) arrays (float64 from an ascii file,
    the stored type from a binary one); header: read_ply_vertex_header(path).  Raises ValueError on
    truncated or malformed data."""
    body, fmt, elements, vi, count, props = header
    pn = [n for n, _ in props]
    if fmt[0] == "ascii":
        tok = body.split()
        skip = sum(e[1] * len(e[2]) for e in elements[:vi])
        need = count * len(props)
        if len(tok) < skip + need:
            raise ValueError(f"{path}: truncated vertex data")
        try:
            rows = np.array(tok[skip:skip + need], dtype=np.float64).reshape(count, len(props))
        except ValueError as e:
            raise ValueError(f"{path}: malformed ascii vertex data") from e
        return [rows[:, pn.index(c)] for c in names]
    off = sum(e[1] * np.dtype([(n, "<" + t) for n, t in e[2]]).itemsize for e in elements[:vi] if e[2])
    dt = np.dtype([(n, "<" + t) for n, t in props])
    if len(body) < off + count * dt.itemsize:
        raise ValueError(f"{path}: truncated vertex data")
    rows = np.frombuffer(body, dtype=dt, count=count, offset=off)
    return [rows[c] for c in names]


def read_ply_xyz(path) -> np.ndarray:
    """The x, y, z properties of a PLY file's vertex element as an (N, 3) float32 array (what
    load_gt_point_cloud takes from plyfile).  Reads `format ascii 1.0` and
    `format binary_little_endian 1.0` with float or double coordinates; the vertex element may carry
    other scalar properties, and other elements may follow it.  Raises ValueError on anything else
    (big-endian data, no vertex element, list properties in or before the vertex element, missing
    or non-floating coordinates, truncated data)."""
    header = read_ply_vertex_header(path)
    props = header[5]
    pn = [n for n, _ in props]
    for c in "xyz":
        if c not in pn:
            raise ValueError(f"{path}: the vertex element has no property {c!r}")
        if dict(props)[c] not in ("f4", "f8"):
            raise ValueError(f"{path}: vertex property {c!r} is not float or double")
    xyz = np.stack(read_ply_vertex_columns(path, header, "xyz"), 1)
    return np.ascontiguousarray(xyz.astype(np.float32))


class GtPointCloud:
    """points: (G, 3) float32 tensor or array (finite, G >= 1); threshold: constraint_treshold.
    Owns the device index and the XY bounds x_min, x_max, y_min, y_max (the fp32 minima and maxima
    of the cloud, as load_gt_point_cloud computes them)."""

    def __init__(self, points, threshold: float = 0.05, device="cuda"):
        self._index = None
        if isinstance(points, torch.Tensor):
            pts = points.detach()
            dev = pts.device if pts.is_cuda else torch.device(device)
        else:
            pts = torch.from_numpy(np.ascontiguousarray(np.asarray(points), dtype=np.float32))
            dev = torch.device(device)
        if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
            raise ValueError(f"points: expected shape (G, 3) with G >= 1, got {tuple(pts.shape)}")
        if pts.dtype != torch.float32:
            raise ValueError("points: expected float32")
        if not bool(torch.isfinite(pts).all()):
            raise ValueError("points: the cloud has a NaN or Inf coordinate")
        self.threshold = float(threshold)
        if not (self.threshold > 0.0 and np.isfinite(self.threshold)):
            raise ValueError("threshold: expected a finite value > 0")
        pts = pts.to(dev).contiguous()
        require_gpu(pts)
        self.device = pts.device
        self.G = int(pts.shape[0])
        L = lib()
        with torch.cuda.device(self.device):
            h = L.gsr_gt_index_create(self.G, ptr(pts), self.threshold, stream(self.device))
        if not h:
            from diff_gaussian_rasterization._lib import last_error
            raise RuntimeError(f"gsr_gt_index_create failed: {last_error()}")
        self._index = ctypes.c_void_p(h)
        b = (ctypes.c_float * 4)()
        check(L.gsr_gt_index_bounds(self._index, b), "gsr_gt_index_bounds")
        self.x_min, self.x_max, self.y_min, self.y_max = (np.float32(v) for v in b)
        info = (ctypes.c_int64 * 6)()
        check(L.gsr_gt_index_info(self._index, info, 6), "gsr_gt_index_info")
        self.cells = int(info[1])
        self.bytes = int(info[2])
        self.grid = (int(info[3]), int(info[4]), int(info[5]))

    @classmethod
    def from_ply(cls, path, threshold: float = 0.05, device="cuda"):
        return cls(read_ply_xyz(path), threshold, device)

    @property
    def handle(self):
        if self._index is None:
            raise RuntimeError("the ground-truth cloud's index has been released")
        return self._index

    def close(self) -> None:
        ix, self._index = self._index, None
        if ix is not None and ix.value:
            lib().gsr_gt_index_destroy(ix)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def far_mask(self, xyz: torch.Tensor, existing_mask: torch.Tensor = None,
                 protected_mask: torch.Tensor = None) -> torch.Tensor:
        """compare_points_to_gt(existing_mask, protected_mask): the bool mask existing | D, with D
        evaluated only on rows in neither mask (scene/gaussian_model.py:853-962)."""
        require_gpu(xyz)
        if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.dtype != torch.float32:
            raise ValueError("xyz: expected (P, 3) float32")
        if xyz.device != self.device:
            raise ValueError("xyz: not on the cloud's device")
        xyz = xyz.detach().contiguous()
        P = xyz.shape[0]
        skip = None
        for m in (existing_mask, protected_mask):
            if m is not None:
                if tuple(m.shape) != (P,) or m.dtype != torch.bool:
                    raise ValueError("masks: expected (P,) bool")
                skip = m if skip is None else skip | m
        skip_u8 = skip.to(device=xyz.device, dtype=torch.uint8).contiguous() if skip is not None else None
        out = torch.empty(P, dtype=torch.uint8, device=xyz.device)
        check(lib().gsr_gt_far_mask(P, ptr(xyz), self.handle, self.threshold, ptr(skip_u8), ptr(out),
                                    stream(xyz.device)), "gsr_gt_far_mask")
        far = out.bool()
        return far if existing_mask is None else existing_mask.to(xyz.device) | far
