"""Fit depth maps of unknown scale to the calibrated sparse points, on the device
(include/gsr_depth_scale.h, csrc/depth_scale.hip).

fit_depth_scales replaces get_scales of the reference's preprocess/make_depth_scale.py (:19-75; README
step "Generate depth_params.json file from the depth maps", run once per chunk by
preprocess/make_chunks_depth_scale.py): per image, the scale and offset that take a 16-bit inverse depth
map -- a monocular network's (preprocess/generate_depth.py), or any PNG a user brings -- onto the inverse
depths of the sparse points the image observes: two medians and two mean absolute deviations over the
image's valid observations.  The rule is stated in gsr_depth_scale.h.

The cameras are chunker.py's qvecs / tvecs, the observations its CSR arrays, and a chunk's call passes
Chunk.obs_index / Chunk.obs_offsets as they are.  The result goes to mesh_depth.write_depth_params
(.params) and to ViewStore.add_depth_maps, DepthMaps.invdepth() and the evaluator (.depth_maps()).

Not here: reading COLMAP models, decoding PNGs (mesh_depth.load_png16 reads the 16-bit greyscale ones),
running a depth network."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List

import numpy as np
import torch

from .chunker import qvec2rotmat
from .mesh_depth import DepthMaps

FITTED, NO_MAP, NAN_SEEN = 1, 2, 4  # GSR_DEPTH_SCALE_*
CAMERA_DOUBLES = 15
RECORD = np.dtype([("scale", "<f8"), ("offset", "<f8"), ("t_colmap", "<f8"), ("s_colmap", "<f8"), ("t_mono", "<f8"),
                   ("s_mono", "<f8"), ("n_valid", "<i4"), ("flags", "<u4")])
_MISSING = {"origin": 0, "skip": 1}


@dataclass
class DepthScaleFit:
    """One entry per fitted camera, in the order of `cameras`.  scale, offset: depth_params.json's
    (0 where the image is not fitted or has no map); n_valid: the valid observations; t_colmap, s_colmap,
    t_mono, s_mono: the medians and mean absolute deviations (0 where not fitted); fitted, nan_seen: bool
    arrays; no_map: the positions (in `cameras`) of the cameras without a map; cameras, map_index: as
    given; bits: the maps on the device, (K, Hd, Wd) int16 holding the uint16 bits (u16: the same as int32
    values 0 .. 65535, DepthMaps.u16's form, made when asked for)."""
    scale: np.ndarray
    offset: np.ndarray
    n_valid: np.ndarray
    t_colmap: np.ndarray
    s_colmap: np.ndarray
    t_mono: np.ndarray
    s_mono: np.ndarray
    fitted: np.ndarray
    nan_seen: np.ndarray
    no_map: List[int]
    cameras: np.ndarray
    map_index: np.ndarray
    bits: torch.Tensor

    @property
    def u16(self) -> torch.Tensor:
        return self.bits.to(torch.int32) & 0xFFFF

    def depth_maps(self) -> DepthMaps:
        """A mesh_depth.DepthMaps with one image per fitted camera, in order: its map with its scale and
        offset.  A camera without a map gets a zero map with scale 0, and so does one whose scale or
        offset is not finite (a flat map): no depth for such a view, as for scale <= 0."""
        n = len(self.cameras)
        dev = self.bits.device
        ok = (self.map_index >= 0) & np.isfinite(self.scale) & np.isfinite(self.offset)
        idx = torch.from_numpy(np.where(ok, self.map_index, 0).astype(np.int64)).to(dev)
        if self.bits.shape[0]:
            u16 = (self.bits[idx].to(torch.int32) & 0xFFFF) * torch.from_numpy(ok.astype(np.int32)).to(dev)[:, None, None]
        else:
            u16 = torch.zeros((n,) + tuple(self.bits.shape[1:]), dtype=torch.int32, device=dev)
        return DepthMaps(u16, np.where(ok, self.scale, 0.0), np.where(ok, self.offset, 0.0))

    def params(self, names) -> dict:
        """{name without extension: (scale, offset)} for mesh_depth.write_depth_params; names: one per
        fitted camera.  Cameras without a map are left out (the reference returns None for them)."""
        names = list(names)
        if len(names) != len(self.cameras):
            raise ValueError("names: expected one per fitted camera")
        return {os.path.splitext(n)[0]: (float(self.scale[k]), float(self.offset[k]))
                for k, n in enumerate(names) if self.map_index[k] >= 0}


def _host(name, a, dtype, tail=()):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype != dtype:
        raise ValueError(f"{name}: expected {np.dtype(dtype).name}, got {a.dtype.name}")
    if a.ndim != 1 + len(tail) or tuple(a.shape[1:]) != tuple(tail):
        raise ValueError(f"{name}: expected shape (n{''.join(', ' + str(s) for s in tail)}), got {a.shape}")
    return np.ascontiguousarray(a)


def _check_large(name, a, dt, tail):
    dtype = str(a.dtype).replace("torch.", "")
    if dtype != dt or len(a.shape) != 1 + len(tail) or tuple(a.shape[1:]) != tail:
        raise ValueError(f"{name}: expected {dt} of shape (n{''.join(', ' + str(v) for v in tail)}), "
                         f"got {dtype} {tuple(a.shape)}")


def camera_table(qvecs, tvecs, sizes, map_index) -> np.ndarray:
    """(M, 15) float64: qvec2rotmat(q) row-major, t, width, height, map index -- R is formed on the host
    in fp64, as the reference forms it."""
    M = len(qvecs)
    out = np.zeros((M, CAMERA_DOUBLES), np.float64)
    for k in range(M):
        out[k, :9] = qvec2rotmat(qvecs[k]).reshape(9)
    out[:, 9:12] = tvecs
    out[:, 12:14] = sizes
    out[:, 14] = map_index
    return out


def _ascending(name, off, total):
    if off.shape[0] < 1 or off[0] != 0 or off[-1] != total or (np.diff(off) < 0).any():
        raise ValueError(f"{name}: expected an ascending sequence from 0 to {total}")


def fit_depth_scales(qvecs, tvecs, sizes, obs_ptr, obs_xy, obs_point_id, point_id, point_xyz, maps, map_index=None,
                     cameras=None, obs_index=None, obs_offsets=None, missing: str = "origin",
                     device="cuda") -> DepthScaleFit:
    """qvecs (M, 4) COLMAP (w, x, y, z), tvecs (M, 3), sizes (M, 2) integers (width, height): the scene's
    cameras (float64 / integer arrays or tensors).  obs_ptr (M + 1) int64, obs_xy (O, 2) float64,
    obs_point_id (O) int64 (-1: none): camera m's observations are rows obs_ptr[m]:obs_ptr[m + 1].
    point_id (N) int64, unique and >= 0; point_xyz (N, 3) float64.  The large arrays (obs_xy,
    obs_point_id, point_id, point_xyz, maps, obs_index) may already be on the device.

    maps: (K, Hd, Wd) -- a tensor in DepthMaps.u16's int32 form or the uint16 bits as int16, or a uint16
    array; one map size per call.  cameras: the cameras to fit (indices into the scene's; default all, in
    order).  map_index: per fitted camera the index of its map or -1 (default: K equals the number of
    fitted cameras and camera k has map k).  obs_index with obs_offsets: Chunk.obs_index / obs_offsets
    -- fitted camera k's observations are obs_index[obs_offsets[k]:obs_offsets[k + 1]], indices into
    obs_xy / obs_point_id; obs_ptr may then be None.  missing: what a point id below max id + 1 without a
    row is: "origin" (the point (0, 0, 0), the reference's) or "skip".

    The id table comes from the chunker's entry points (which synchronise to report a duplicate id); the
    fit itself is one launch for the batch and the host waits only to copy the records back."""
    if missing not in _MISSING:
        raise ValueError("missing: expected 'origin' or 'skip'")
    obs_xy, obs_point_id, point_id, point_xyz = (a if isinstance(a, torch.Tensor) else np.asarray(a)
                                                 for a in (obs_xy, obs_point_id, point_id, point_xyz))
    q = _host("qvecs", qvecs, np.float64, (4,))
    t = _host("tvecs", tvecs, np.float64, (3,))
    M = q.shape[0]
    if t.shape[0] != M:
        raise ValueError("qvecs, tvecs: expected as many quaternions as translations")
    sz = np.asarray(sizes.detach().cpu().numpy() if isinstance(sizes, torch.Tensor) else sizes)
    if sz.shape != (M, 2) or not np.issubdtype(sz.dtype, np.integer):
        raise ValueError(f"sizes: expected ({M}, 2) integers (width, height), got {sz.shape} {sz.dtype.name}")
    if M and (sz.min() < 1 or sz.max() > 1 << 24):
        raise ValueError("sizes: expected 1 <= width, height <= 2^24")
    for name, a, dt, tail in (("obs_xy", obs_xy, "float64", (2,)), ("obs_point_id", obs_point_id, "int64", ()),
                              ("point_id", point_id, "int64", ()), ("point_xyz", point_xyz, "float64", (3,))):
        _check_large(name, a, dt, tail)
    O, N = int(obs_point_id.shape[0]), int(point_id.shape[0])
    if obs_xy.shape[0] != O:
        raise ValueError("obs_xy, obs_point_id: expected one row per observation in each")
    if point_xyz.shape[0] != N:
        raise ValueError("point_id, point_xyz: expected one row per point in each")
    if N >= 2 ** 31:
        raise ValueError("point_id: expected fewer than 2^31 points")

    if cameras is None:
        cams = np.arange(M, dtype=np.int64)
    else:
        cams = _host("cameras", cameras, np.int64)
        if cams.size and (cams.min() < 0 or cams.max() >= M):
            raise ValueError(f"cameras: expected indices in [0, {M})")
    F = cams.shape[0]

    mdt = str(maps.dtype).replace("torch.", "")
    if len(maps.shape) != 3 or mdt not in ("int32", "int16", "uint16"):
        raise ValueError(f"maps: expected (K, Hd, Wd) int32 values, int16 bits or uint16, got {tuple(maps.shape)} {mdt}")
    K, Hd, Wd = (int(v) for v in maps.shape)
    if Hd < 1 or Wd < 1:
        raise ValueError(f"maps: expected Hd, Wd >= 1, got {Hd} x {Wd}")
    if Hd > 32768 or Wd > 32768:
        raise ValueError("maps: expected Hd, Wd <= 32768")
    if map_index is None:
        if K != F:
            raise ValueError(f"maps: {K} maps for {F} cameras and no map_index")
        mi = np.arange(F, dtype=np.int64)
    else:
        mi = _host("map_index", map_index, np.int64)
        if mi.shape[0] != F:
            raise ValueError(f"map_index: expected one entry per fitted camera ({F}), got {mi.shape[0]}")
        if mi.size and (mi.min() < -1 or mi.max() >= K):
            raise ValueError(f"map_index: expected -1 or an index in [0, {K})")

    if (obs_index is None) != (obs_offsets is None):
        raise ValueError("obs_index, obs_offsets: expected both or neither")
    if obs_index is not None:
        if not isinstance(obs_index, torch.Tensor):
            obs_index = np.asarray(obs_index)
        _check_large("obs_index", obs_index, "int64", ())
        off = _host("obs_offsets", obs_offsets, np.int64)
        if off.shape[0] != F + 1:
            raise ValueError(f"obs_offsets: expected {F + 1} entries for {F} cameras, got {off.shape[0]}")
        _ascending("obs_offsets", off, int(obs_index.shape[0]))
        ptr_host = None
    else:
        ptr_host = _host("obs_ptr", obs_ptr, np.int64)
        if ptr_host.shape[0] != M + 1:
            raise ValueError(f"obs_ptr: expected {M + 1} entries for {M} cameras, got {ptr_host.shape[0]}")
        _ascending("obs_ptr", ptr_host, O)
        off = None

    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("gs_train kernels require a ROCm GPU device")
    for a in (obs_xy, obs_point_id, point_id, point_xyz, maps, obs_index):
        if isinstance(a, torch.Tensor) and a.is_cuda:
            dev = a.device
            break

    import ctypes

    from ._native import check, lib, ptr, stream
    from .chunker import _dev
    L = lib()
    xy_d, pid_d, id_d, xyz_d = (_dev(a, dev) for a in (obs_xy, obs_point_id, point_id, point_xyz))
    if isinstance(maps, torch.Tensor):
        m = maps.detach().to(dev)
        bits = (m & 0xFFFF).to(torch.int16).contiguous() if m.dtype == torch.int32 else m.contiguous()
    else:
        bits = torch.from_numpy(np.ascontiguousarray(np.asarray(maps).view(np.int16))).to(dev)

    if obs_index is not None:
        index_d, off_host = _dev(obs_index, dev), off
    elif cameras is None:
        index_d, off_host = None, ptr_host
    else:  # a subset without an index: its ranges of the arrays, one after the other
        counts = ptr_host[cams + 1] - ptr_host[cams]
        off_host = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        shift = torch.from_numpy(ptr_host[cams] - off_host[:-1]).to(dev)
        index_d = torch.arange(int(off_host[-1]), dtype=torch.int64, device=dev) + \
            torch.repeat_interleave(shift, torch.from_numpy(counts).to(dev))
    Lobs = int(off_host[-1])

    table_h = camera_table(q[cams], t[cams], sz[cams], mi)
    records = torch.zeros(F * RECORD.itemsize, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        s = stream(dev)
        mm = (ctypes.c_int64 * 2)()
        check(L.gsr_chunk_id_range(N, ptr(id_d), mm, s), "gsr_chunk_id_range")
        if N and mm[0] < 0:
            raise ValueError(f"point_id: a negative id ({mm[0]})")
        if N and mm[1] >= 2 ** 31 - 1:
            raise ValueError(f"point_id: the largest id ({mm[1]}) must be below 2^31 - 1")
        T = int(mm[1]) + 1 if N else 0
        table = torch.empty(T, dtype=torch.int32, device=dev)
        check(L.gsr_chunk_id_table(N, ptr(id_d), T, ptr(table), s), "gsr_chunk_id_table")
        cams_d, off_d = torch.from_numpy(table_h).to(dev), torch.from_numpy(off_host).to(dev)
        scratch = torch.empty(max(int(L.gsr_depth_scale_scratch_bytes(Lobs)), 16), dtype=torch.uint8, device=dev)
        check(L.gsr_depth_scale_fit(F, ptr(cams_d), ptr(off_d), Lobs, ptr(index_d), O, ptr(xy_d), ptr(pid_d), N, T,
                                    ptr(table), ptr(xyz_d), K, Hd, Wd, ptr(bits), _MISSING[missing], ptr(scratch),
                                    ptr(records), s), "gsr_depth_scale_fit")
        rec = records.cpu().numpy().view(RECORD)  # the call's one wait on the device
    flags = rec["flags"]
    return DepthScaleFit(rec["scale"].copy(), rec["offset"].copy(), rec["n_valid"].astype(np.int64),
                         rec["t_colmap"].copy(), rec["s_colmap"].copy(), rec["t_mono"].copy(), rec["s_mono"].copy(),
                         (flags & FITTED) != 0, (flags & NAN_SEEN) != 0,
                         [int(k) for k in np.nonzero(mi < 0)[0]], cams, mi, bits)
