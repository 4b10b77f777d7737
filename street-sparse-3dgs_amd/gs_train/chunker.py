"""The scene partition on the device (include/gsr_chunker.h, csrc/chunker.hip).

partition_scene replaces make_chunk and the grid set-up of the reference's chunker
(preprocess/ss_make_chunk.py:441-643, 671-747) from the decoded calibration on: which cameras train a
chunk, which sparse points seed it, which 2-D observations each image keeps and which depth-only views
belong to it.  The reference answers these per chunk in Python; the chunk boxes tile the plane, so here
one classification of the points and one histogram per camera answer them for every chunk at once, and
the host only resolves the random draws.  A chunk's `center` and `extent` are what prepare_chunk_cloud
(gs_train/lidar.py) takes.

The rule is stated in gsr_chunker.h.  The reference script cannot be run beside this project, so parity
with it is unpinned: the tests hold the device to a literal per-chunk restatement of the rule.

Not here: COLMAP model files (read_write_model), images_depths.bin, the new ids of LiDAR points
(max_id + k + 1, one line for the caller) and blending_dict.json's file form."""
from __future__ import annotations

import contextlib
import ctypes
import random
import time
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

IN, NEAR, DRAW = 1, 2, 3      # GSR_CHUNK_IN / _NEAR / _DRAW
NOT_IN_C = -2                 # GSR_CHUNK_NOT_IN_C: cell32 of a row with error >= 10 (or NaN)
FAR = 1e12


def qvec2rotmat(q):
    """COLMAP's rotation matrix of a quaternion (w, x, y, z), in the dtype of q."""
    w, x, y, z = q
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def camera_centers(qvecs, tvecs, dtype=np.float32) -> np.ndarray:
    """(M, 3) centres -R.T @ t, with R (formed in fp64) and t cast to dtype first: float32 for the
    training cameras (:675-678), float64 for the depth-only ones (:567)."""
    q = np.asarray(qvecs, dtype=np.float64).reshape(-1, 4)
    t = np.asarray(tvecs, dtype=np.float64).reshape(-1, 3)
    if len(q) != len(t):
        raise ValueError("qvecs, tvecs: expected as many quaternions as translations")
    out = np.zeros((len(q), 3), dtype=dtype)
    for k in range(len(q)):
        out[k] = -qvec2rotmat(q[k]).astype(dtype).T @ t[k].astype(dtype)
    return out


def chunk_grid(cam_centers, chunk_size: float = 100.0, min_padd: float = 0.2):
    """(global_bbox (2, 3) float32, n_w, n_h): the cameras' bounding box padded by min_padd chunk_size and
    then to a whole number of chunks, all in float32 (:720-736); z is -+1e12."""
    cam = np.asarray(cam_centers, dtype=np.float32)
    if cam.ndim != 2 or cam.shape[1] != 3 or cam.shape[0] < 1:
        raise ValueError("cam_centers: expected (M, 3) with M >= 1")
    chunk_size = float(chunk_size)
    if not (chunk_size > 0.0 and np.isfinite(chunk_size)):
        raise ValueError("chunk_size: expected a finite value > 0")
    cs = np.float32(chunk_size)
    pad = np.float32(float(min_padd) * chunk_size)
    bbox = np.stack([cam.min(axis=0), cam.max(axis=0)]).astype(np.float32)
    if not np.isfinite(bbox).all():
        raise ValueError("cam_centers: a centre has a NaN or Inf coordinate")
    bbox[0, :2] -= pad
    bbox[1, :2] += pad
    extent = bbox[1] - bbox[0]
    padd = np.array([cs - extent[0] % cs, cs - extent[1] % cs], dtype=np.float32)
    bbox[0, :2] -= padd / np.float32(2)
    bbox[1, :2] += padd / np.float32(2)
    bbox[0, 2] = -FAR
    bbox[1, 2] = FAR
    extent = bbox[1] - bbox[0]
    n_w = int(round(float(np.float32(extent[0] / cs))))
    n_h = int(round(float(np.float32(extent[1] / cs))))
    return bbox, n_w, n_h


def cell_bounds(bbox, chunk_size, i, j):
    """(lo, hi), fp64: box(i, j) of gsr_chunker.h; bx(i) = x0 + i cs, one rounded product and sum."""
    x0, y0, cs = float(bbox[0][0]), float(bbox[0][1]), float(chunk_size)
    return (np.array([x0 + i * cs, y0 + j * cs, -FAR]), np.array([x0 + (i + 1) * cs, y0 + (j + 1) * cs, FAR]))


def _check_grid(bbox, n_w, n_h, chunk_size):
    n_w, n_h = int(n_w), int(n_h)
    if n_w < 1 or n_h < 1 or n_w * n_h >= 2 ** 31:
        raise ValueError(f"grid: expected 1 <= n_w, n_h and n_w n_h < 2^31, got {n_w} x {n_h}")
    lo, _ = cell_bounds(bbox, chunk_size, 0, 0)
    hi, _ = cell_bounds(bbox, chunk_size, n_w, n_h)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and -FAR < lo[0] and -FAR < lo[1] and hi[0] < FAR
            and hi[1] < FAR):
        raise ValueError("grid: the bounds must be finite and inside +-1e12")
    return n_w, n_h


def resolve_candidates(candidates, cells: int, min_n_cams: int = 5, max_n_cams: int = 1500, rng=None):
    """The host half of the camera rule.  candidates: (K, 5) rows (cell, m, state, n_pts, total) sorted by
    (cell, m).  Per cell in order, with the one `rng` (default random.Random(0)): a DRAW camera is valid
    iff rng.uniform(0, 0.5) < n_pts / total (:493); while more than max_n_cams are valid, as many times
    as there were too many, rng.randint(0, count - 1) picks the valid camera to remove, counted in
    ascending index (:497-501); the chunk is emitted iff count > min_n_cams (:507).  The draws happen for
    excluded chunks too.  Returns a list over the cells of (cameras int64 array, emitted)."""
    rng = random.Random(0) if rng is None else rng
    cand = np.asarray(candidates, dtype=np.int64).reshape(-1, 5)
    first = np.searchsorted(cand[:, 0], np.arange(cells + 1))
    out = []
    for cell in range(cells):
        valid = []
        for _, m, state, n, total in cand[first[cell]:first[cell + 1]].tolist():
            if state != DRAW or rng.uniform(0, 0.5) < float(n) / total:
                valid.append(m)
        for _ in range(len(valid) - max_n_cams):
            del valid[rng.randint(0, len(valid) - 1)]
        out.append((np.array(valid, dtype=np.int64), len(valid) > min_n_cams))
    return out


def fill_temporal_gaps(selected, order, xy, max_gap: float = 10.0) -> set:
    """fill_temporal_gaps_in_chunk (:391-437).  selected: the recordings (rows of xy) of a chunk's
    depth-only views; order: the recordings sorted by time (order[k] is the k-th in time); xy: (R, 2)
    recording positions.  A recording next in time to a selected one, across a gap in the selection, is
    added when it lies closer than max_gap to it: for every selected one but the last, its predecessor
    (not for the first) and its successor; then the one before the first and the one after the last.
    The last selected recording's predecessor is never examined, as in the reference.  Selected
    recordings missing from `order` are ignored.  Returns the set of added recordings."""
    order = [int(v) for v in order]
    xy = np.asarray(xy, dtype=np.float64)
    rank = {r: k for k, r in enumerate(order)}
    ci = sorted({rank[int(s)] for s in selected if int(s) in rank})
    added = set()
    if not ci:
        return added

    def close(a, b):
        d = xy[order[a]] - xy[order[b]]
        return np.sqrt(d[0] ** 2 + d[1] ** 2) < max_gap

    for k in range(len(ci) - 1):
        cur = ci[k]
        if k > 0 and cur - ci[k - 1] > 1 and close(cur, cur - 1):
            added.add(order[cur - 1])
        if ci[k + 1] - cur > 1 and close(cur, cur + 1):
            added.add(order[cur + 1])
    if ci[0] > 0 and close(ci[0] - 1, ci[0]):
        added.add(order[ci[0] - 1])
    if ci[-1] < len(order) - 1 and close(ci[-1], ci[-1] + 1):
        added.add(order[ci[-1] + 1])
    return added


@dataclass
class Chunk:
    """One emitted chunk.  center / extent: (lo + hi) / 2 and hi - lo of its box, fp64 (center.txt,
    extent.txt; z gives 0 and 2e12).  cameras: the selected cameras, ascending.  obs_index: the kept
    observations of those cameras as indices into obs_point_id, camera after camera in their original
    order; camera k's are obs_index[obs_offsets[k]:obs_offsets[k + 1]].  points: the rows of the point
    arrays that seed the chunk, in input order.  blend: per selected camera, its observations of this
    chunk's points.  depth_cameras: the depth-only cameras centred in the box."""
    i: int
    j: int
    center: np.ndarray
    extent: np.ndarray
    cameras: np.ndarray
    obs_offsets: np.ndarray
    obs_index: torch.Tensor
    points: torch.Tensor
    blend: np.ndarray
    depth_cameras: np.ndarray


@dataclass
class ScenePartition:
    """global_bbox, n_w, n_h, chunk_size: the grid (cell (i, j) has the index i n_h + j).  chunks: the
    emitted chunks in cell order; excluded: the (i, j) of the others.  For inspection, on the device:
    n_pts / blend (M, cells) and total (M) int32, cell32 / cell64 (N) int32 (cell32 is NOT_IN_C for a row
    with error >= 10), cam_cell (M) and depth_cell (D); candidates: the (K, 5) host array of
    (cell, m, state, n_pts, total)."""
    global_bbox: np.ndarray
    n_w: int
    n_h: int
    chunk_size: float
    chunks: List[Chunk] = field(default_factory=list)
    excluded: List[tuple] = field(default_factory=list)
    n_pts: Optional[torch.Tensor] = None
    total: Optional[torch.Tensor] = None
    blend: Optional[torch.Tensor] = None
    cell32: Optional[torch.Tensor] = None
    cell64: Optional[torch.Tensor] = None
    cam_cell: Optional[torch.Tensor] = None
    depth_cell: Optional[torch.Tensor] = None
    candidates: Optional[np.ndarray] = None


def _host(name, a, dtype, shape_tail=()):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype != dtype:
        raise ValueError(f"{name}: expected {np.dtype(dtype).name}, got {a.dtype.name}")
    if a.ndim != 1 + len(shape_tail) or tuple(a.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"{name}: expected shape (n{''.join(', ' + str(s) for s in shape_tail)}), got {a.shape}")
    return np.ascontiguousarray(a)


def _check_inputs(cam_centers, obs_ptr, obs_point_id, point_id, point_xyz, point_error, depth_centers):
    """Types, shapes and the observation ranges; what needs the device (duplicate ids) is checked there."""
    cam = _host("cam_centers", cam_centers, np.float32, (3,))
    ptr_ = _host("obs_ptr", obs_ptr, np.int64)
    M = cam.shape[0]
    if ptr_.shape[0] != M + 1:
        raise ValueError(f"obs_ptr: expected {M + 1} entries for {M} cameras, got {ptr_.shape[0]}")
    for name, a, dt, tail in (("obs_point_id", obs_point_id, "int64", ()), ("point_id", point_id, "int64", ()),
                              ("point_xyz", point_xyz, "float64", (3,)), ("point_error", point_error, "float32", ())):
        dtype = str(a.dtype).replace("torch.", "")
        if dtype != dt or len(a.shape) != 1 + len(tail) or tuple(a.shape[1:]) != tail:
            raise ValueError(f"{name}: expected {dt} of shape (n{''.join(', ' + str(v) for v in tail)}), "
                             f"got {dtype} {tuple(a.shape)}")
    O, N = int(obs_point_id.shape[0]), int(point_id.shape[0])
    if point_xyz.shape[0] != N or point_error.shape[0] != N:
        raise ValueError("point_id, point_xyz, point_error: expected one row per point in each")
    if N >= 2 ** 31:
        raise ValueError("point_id: expected fewer than 2^31 points")
    if ptr_[0] != 0 or ptr_[-1] != O or (np.diff(ptr_) < 0).any():
        raise ValueError("obs_ptr: expected an ascending sequence from 0 to len(obs_point_id)")
    depth = None
    if depth_centers is not None:
        depth = _host("depth_centers", depth_centers, np.float64, (3,))
    return cam, ptr_, depth


# tools/chunker_bench.py sets this to a dict: each stage of partition_scene is then bracketed by device
# synchronisations and its wall-clock milliseconds are appended under its name
_STAGE_TIMES = None


@contextlib.contextmanager
def _stage(name, dev):
    if _STAGE_TIMES is None:
        yield
        return
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize(dev)
    _STAGE_TIMES.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)


def _dev(a, device):
    if isinstance(a, torch.Tensor):
        return a.detach().to(device).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a))).to(device)


def partition_scene(cam_centers, obs_ptr, obs_point_id, point_id, point_xyz, point_error, depth_centers=None,
                    chunk_size: float = 100.0, min_padd: float = 0.2, min_n_cams: int = 5, max_n_cams: int = 1500,
                    add_far_cams: bool = True, rng=None, device="cuda", grid=None) -> ScenePartition:
    """cam_centers: (M, 3) float32 (camera_centers); obs_ptr: (M + 1) int64, camera m's observations are
    obs_point_id[obs_ptr[m]:obs_ptr[m + 1]] (int64 point ids, -1: none); point_id (N) int64, unique and
    >= 0; point_xyz (N, 3) float64; point_error (N) float32; depth_centers: (D, 3) float64 or None.
    Arrays or tensors; the large ones may already be on the device.  rng: the random.Random the draws
    come from, default random.Random(0).  grid: (global_bbox, n_w, n_h) instead of chunk_grid's (a scene
    without cameras has no grid of its own)."""
    obs_point_id, point_id, point_xyz, point_error = (a if isinstance(a, torch.Tensor) else np.asarray(a) for a in
                                                      (obs_point_id, point_id, point_xyz, point_error))
    cam, ptr_host, depth = _check_inputs(cam_centers, obs_ptr, obs_point_id, point_id, point_xyz, point_error,
                                         depth_centers)
    chunk_size = float(chunk_size)
    if not (chunk_size > 0.0 and np.isfinite(chunk_size)):
        raise ValueError("chunk_size: expected a finite value > 0")
    if grid is None:
        if cam.shape[0] == 0:
            raise ValueError("cam_centers: no cameras and no grid given")
        grid = chunk_grid(cam, chunk_size, min_padd)
    bbox = np.asarray(grid[0], dtype=np.float32)
    n_w, n_h = _check_grid(bbox, grid[1], grid[2], chunk_size)
    cells = n_w * n_h
    M, N, O = cam.shape[0], int(point_id.shape[0]), int(obs_point_id.shape[0])
    D = 0 if depth is None else depth.shape[0]
    if M * cells >= 2 ** 31:
        raise ValueError(f"cameras x cells must stay below 2^31, got {M} x {cells}")

    from diff_gaussian_rasterization._lib import ChunkGrid
    from ._native import check, lib, ptr, stream
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("gs_train kernels require a ROCm GPU device")
    L = lib()
    g = ChunkGrid(float(bbox[0, 0]), float(bbox[0, 1]), chunk_size, n_w, n_h)
    i32 = dict(dtype=torch.int32, device=dev)
    cam_d, ptr_d = _dev(cam, dev), _dev(ptr_host, dev)
    obs_d, id_d, xyz_d, err_d = (_dev(a, dev) for a in (obs_point_id, point_id, point_xyz, point_error))
    depth_d = _dev(depth, dev) if D else None
    part = ScenePartition(bbox, n_w, n_h, chunk_size)
    with torch.cuda.device(dev):
        s = stream(dev)
        with _stage("classify_points", dev):
            cell32, cell64 = torch.empty(N, **i32), torch.empty(N, **i32)
            check(L.gsr_chunk_classify_points(N, ptr(xyz_d), ptr(err_d), ctypes.byref(g), ptr(cell32), ptr(cell64), s),
                  "gsr_chunk_classify_points")
        with _stage("classify_centers", dev):
            cam_cell, depth_cell = torch.empty(M, **i32), torch.empty(D, **i32)
            check(L.gsr_chunk_classify_centers(M, ptr(cam_d), D, ptr(depth_d), ctypes.byref(g), ptr(cam_cell),
                                               ptr(depth_cell), s), "gsr_chunk_classify_centers")
        with _stage("id_table", dev):
            mm = (ctypes.c_int64 * 2)()
            check(L.gsr_chunk_id_range(N, ptr(id_d), mm, s), "gsr_chunk_id_range")
            if N and mm[0] < 0:
                raise ValueError(f"point_id: a negative id ({mm[0]})")
            if N and mm[1] >= 2 ** 31 - 1:
                raise ValueError(f"point_id: the largest id ({mm[1]}) must be below 2^31 - 1")
            T = int(mm[1]) + 1 if N else 0
            table = torch.empty(T, **i32)
            check(L.gsr_chunk_id_table(N, ptr(id_d), T, ptr(table), s), "gsr_chunk_id_table")
        with _stage("camera_counts", dev):
            n_pts, blend = torch.empty((M, cells), **i32), torch.empty((M, cells), **i32)
            total = torch.empty(M, **i32)
            check(L.gsr_chunk_camera_counts(M, ptr(ptr_d), O, ptr(obs_d), T, ptr(table), ptr(cell32), ptr(xyz_d), cells,
                                            ptr(n_pts), ptr(blend), ptr(total), s), "gsr_chunk_camera_counts")
        with _stage("candidates", dev):
            scratch = torch.empty(max(int(L.gsr_chunk_candidates_scratch_bytes(M * cells)), 1), dtype=torch.uint8,
                                  device=dev)
            k = ctypes.c_int64(0)
            check(L.gsr_chunk_candidates_count(M, ptr(cam_d), ptr(cam_cell), ptr(n_pts), ctypes.byref(g),
                                               int(add_far_cams), ptr(scratch), ctypes.byref(k), s),
                  "gsr_chunk_candidates_count")
            cand_d = torch.empty((int(k.value), 5), **i32)
            if k.value:
                check(L.gsr_chunk_candidates_write(M, ptr(cam_d), ptr(cam_cell), ptr(n_pts), ptr(total), ctypes.byref(g),
                                                   int(add_far_cams), ptr(scratch), ptr(cand_d), s),
                      "gsr_chunk_candidates_write")
            cand = cand_d.cpu().numpy()
        # the host's draws, then the observation filter of the emitted chunks' cameras
        with _stage("host_draws", dev):
            resolved = resolve_candidates(cand, cells, min_n_cams, max_n_cams, rng)
            emitted = [c for c in range(cells) if resolved[c][1]]
            pair_cell = np.concatenate([np.full(len(resolved[c][0]), c, np.int32) for c in emitted]
                                       + [np.zeros(0, np.int32)])
            pair_cam = np.concatenate([resolved[c][0].astype(np.int32) for c in emitted] + [np.zeros(0, np.int32)])
            P = len(pair_cell)
        with _stage("obs_filter", dev):
            pc_d, pm_d = _dev(pair_cell, dev), _dev(pair_cam, dev)
            scratch = torch.empty(max(int(L.gsr_chunk_obs_filter_scratch_bytes(P)), 1), dtype=torch.uint8, device=dev)
            offsets = torch.empty(P + 1, dtype=torch.int64, device=dev)
            kept = ctypes.c_int64(0)
            check(L.gsr_chunk_obs_filter_count(P, ptr(pc_d), ptr(pm_d), M, ptr(ptr_d), O, ptr(obs_d), T, ptr(table),
                                               ptr(cell64), ptr(scratch), ptr(offsets), ctypes.byref(kept), s),
                  "gsr_chunk_obs_filter_count")
            obs_index = torch.empty(int(kept.value), dtype=torch.int64, device=dev)
            check(L.gsr_chunk_obs_filter_write(P, ptr(pc_d), ptr(pm_d), M, ptr(ptr_d), O, ptr(obs_d), T, ptr(table),
                                               ptr(cell64), ptr(offsets), ptr(obs_index), s),
                  "gsr_chunk_obs_filter_write")
        with _stage("points_by_cell", dev):
            scratch = torch.empty(max(int(L.gsr_chunk_points_by_cell_scratch_bytes(N, cells)), 1), dtype=torch.uint8,
                                  device=dev)
            rows = torch.empty(N, **i32)
            row_off = torch.empty(cells + 1, dtype=torch.int64, device=dev)
            check(L.gsr_chunk_points_by_cell(N, ptr(cell32), cells, ptr(scratch), ptr(rows), ptr(row_off), s),
                  "gsr_chunk_points_by_cell")
            del scratch
        offsets_h, row_off_h = offsets.cpu().numpy(), row_off.cpu().numpy()
        depth_cell_h = depth_cell.cpu().numpy()
        blend_h = blend[_dev(pair_cam.astype(np.int64), dev), _dev(pair_cell.astype(np.int64), dev)].cpu().numpy() \
            if P else np.zeros(0, np.int32)

    p0 = 0
    for c in range(cells):
        i, j = divmod(c, n_h)
        cams, ok = resolved[c]
        if not ok:
            part.excluded.append((i, j))
            continue
        lo, hi = cell_bounds(bbox, chunk_size, i, j)
        p1 = p0 + len(cams)
        off = offsets_h[p0:p1 + 1]
        part.chunks.append(Chunk(i, j, (lo + hi) / 2, hi - lo, cams, off - off[0], obs_index[int(off[0]):int(off[-1])],
                                 rows[int(row_off_h[c]):int(row_off_h[c + 1])].long(), blend_h[p0:p1].copy(),
                                 np.nonzero(depth_cell_h == c)[0].astype(np.int64)))
        p0 = p1
    part.n_pts, part.total, part.blend = n_pts, total, blend
    part.cell32, part.cell64, part.cam_cell, part.depth_cell = cell32, cell64, cam_cell, depth_cell
    part.candidates = cand
    return part
