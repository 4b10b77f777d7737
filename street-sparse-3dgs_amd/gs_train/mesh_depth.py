"""A chunk's depth supervision maps on the device (include/gsr_mesh_depth.h, csrc/mesh_depth.hip).

Replaces steps 7 and 8 of the reference's ss_utils/ss_generate_depths.py: render_mesh_distance is the
ray cast of the reconstructed mesh from every camera (render_depth_gaussians, an embree binary in a
container there), encode_depth_maps is ss_utils/depth_scripts/depth_map_to_distances.py -- the
3-channel distance code's quantisation, the 16-bit normalised inverse depth map and the per-image
scale / offset of depth_params.json -- and DepthMaps.invdepth() is what scene/cameras.py:71-88 makes
of them again: the train step's mono_invdepths / depth_masks and the evaluator's invdepthmap.

The mesh is what lidar.read_ply_mesh returns, the cameras are chunker.py's qvecs / tvecs.  The rule
is stated in gsr_mesh_depth.h; LAZ, .ctm and .stations files, vis2mesh itself and the face directions
of augment_recording_details.py stay with the caller."""
from __future__ import annotations

import ctypes
import json
import os
import struct
import zlib
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from ._native import check, lib, ptr, require_gpu, stream
from .lidar import _device_rows

_MAX_PAIRS = 1 << 27  # (camera, triangle) pairs per call: 1 GiB of counts and offsets


def _camera_table(qvecs, tvecs, intrinsics) -> np.ndarray:
    q = np.asarray(qvecs.detach().cpu() if isinstance(qvecs, torch.Tensor) else qvecs, dtype=np.float64)
    t = np.asarray(tvecs.detach().cpu() if isinstance(tvecs, torch.Tensor) else tvecs, dtype=np.float64)
    k = np.asarray(intrinsics.detach().cpu() if isinstance(intrinsics, torch.Tensor) else intrinsics, dtype=np.float64)
    if q.ndim != 2 or q.shape[1] != 4:
        raise ValueError(f"qvecs: expected (K, 4), got {q.shape}")
    if t.shape != (q.shape[0], 3):
        raise ValueError(f"tvecs: expected ({q.shape[0]}, 3), got {t.shape}")
    if k.shape == (4,):
        k = np.broadcast_to(k, (q.shape[0], 4))
    if k.shape != (q.shape[0], 4):
        raise ValueError(f"intrinsics: expected (K, 4) fx, fy, cx, cy (or one row for all), got {k.shape}")
    return np.ascontiguousarray(np.concatenate([q, t, k], 1))


def render_mesh_distance(vertices, faces, qvecs, tvecs, intrinsics, W: int, H: int, tnear: float = 0.0,
                         tfar: float = 1000.0, depth: str = "ray", device="cuda", stats: Optional[dict] = None):
    """(K, H, W) float32 on the device: per pixel the distance to the nearest triangle of the mesh, 0
    where the pixel's ray hits none.  vertices (V, 3) float32, faces (F, 3) int32; qvecs (K, 4) COLMAP
    (w, x, y, z), tvecs (K, 3) with x_cam = R x + t, intrinsics (K, 4) or (4,) fx, fy, cx, cy (tensors
    or arrays).  The ray of pixel (ix, iy) goes through (ix + 0.5, iy + 0.5); hits count for
    tnear < distance <= tfar (tfar = 1000 is the reference's).  depth="ray": the distance along the
    ray, which is what the reference renders; depth="z": the camera z of the same hit, which is what
    the rasterizer's inverse depth is the reciprocal of.  Faces with an index out of range or a
    non-finite vertex are skipped.

    The reference renders 1536 x 1536 and keeps every third sample, so its sample of output pixel ix
    sits at ix + 1/6: a caller who wants that passes cx + 1/3, cy + 1/3.

    stats: a dict that receives the binning's figures (references, oversize, longest_run,
    occupied_tiles, and bin_us / cast_us, the microseconds between device events around the binning and
    the ray cast; summed over the camera batches, longest_run their maximum)."""
    if depth not in ("ray", "z"):
        raise ValueError("depth: expected 'ray' or 'z'")
    W, H = int(W), int(H)
    if W < 0 or H < 0 or W > 32768 or H > 32768:
        raise ValueError("W, H: expected 0 .. 32768")
    tnear, tfar = float(tnear), float(tfar)
    if not (0.0 <= tnear < tfar and np.isfinite(np.float32(tfar))):
        raise ValueError("tnear, tfar: expected 0 <= tnear < tfar, finite")
    for a in (vertices, faces):
        if isinstance(a, torch.Tensor):
            require_gpu(a)
    dev = vertices.device if isinstance(vertices, torch.Tensor) else torch.device(device)
    v = _device_rows("vertices", vertices, dev)
    f = _device_rows("faces", faces, dev, torch.int32)
    cams = _camera_table(qvecs, tvecs, intrinsics)
    K, F = cams.shape[0], f.shape[0]
    out = torch.empty((K, H, W), dtype=torch.float32, device=dev)
    if K == 0 or W == 0 or H == 0:
        return out
    if F == 0 or v.shape[0] == 0:
        return out.zero_()
    L = lib()
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    per_call = max(1, min(K, _MAX_PAIRS // F, ((1 << 31) - 1) // tiles))
    if per_call * F >= (1 << 31):
        raise ValueError("faces: too many triangles for one camera (F < 2^31)")
    cams_d = torch.from_numpy(cams).to(dev)
    scratch = torch.empty(L.gsr_mesh_distance_scratch_bytes(per_call, F), dtype=torch.uint8, device=dev)
    st = (ctypes.c_int64 * 6)()
    total = {"references": 0, "oversize": 0, "longest_run": 0, "occupied_tiles": 0, "bin_us": 0, "cast_us": 0}
    with torch.cuda.device(dev):
        for k0 in range(0, K, per_call):
            n = min(per_call, K - k0)
            check(L.gsr_mesh_distance_maps(v.shape[0], ptr(v), F, ptr(f), n, ptr(cams_d[k0:k0 + n]), W, H, tnear, tfar,
                                           1 if depth == "z" else 0, ptr(scratch), ptr(out[k0:k0 + n]),
                                           st if stats is not None else None, stream(dev)),
                  "gsr_mesh_distance_maps")
            total["references"] += int(st[0])
            total["oversize"] += int(st[1])
            total["longest_run"] = max(total["longest_run"], int(st[2]))
            total["occupied_tiles"] += int(st[3])
            total["bin_us"] += int(st[4])
            total["cast_us"] += int(st[5])
    if stats is not None:
        stats.update(total)
    return out


# ---- 16-bit greyscale PNG (zlib and struct only) -------------------------------------------------------

_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def _png_chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def save_png16(path, image) -> None:
    """Write a (H, W) uint16 array as a 16-bit greyscale PNG (filter 0 on every row, no interlace)."""
    a = np.asarray(image)
    if a.ndim != 2 or a.dtype != np.uint16 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"image: expected (H, W) uint16 with H, W >= 1, got {a.shape} {a.dtype}")
    H, W = a.shape
    rows = np.zeros((H, 1 + 2 * W), np.uint8)
    rows[:, 1:] = a.astype(">u2").view(np.uint8).reshape(H, 2 * W)
    data = _PNG_MAGIC + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 16, 0, 0, 0, 0)) + \
        _png_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _png_chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(data)


def _paeth(a, b, c):
    p = a.astype(np.int32) + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c)).astype(np.uint8)


def load_png16(path) -> np.ndarray:
    """Read a 16-bit greyscale, non-interlaced PNG (any row filters) as (H, W) uint16.  Every chunk's
    CRC is checked.  Raises ValueError on anything else."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != _PNG_MAGIC:
        raise ValueError(f"{path}: not a PNG")
    pos, head, idat, ended = 8, None, [], False
    while pos + 12 <= len(raw) and not ended:
        (n,) = struct.unpack(">I", raw[pos:pos + 4])
        kind, data = raw[pos + 4:pos + 8], raw[pos + 8:pos + 8 + n]
        if len(data) != n or pos + 12 + n > len(raw):
            raise ValueError(f"{path}: truncated chunk")
        (crc,) = struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])
        if crc != (zlib.crc32(kind + data) & 0xFFFFFFFF):
            raise ValueError(f"{path}: bad CRC in chunk {kind!r}")
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", data)
        elif kind == b"IDAT":
            idat.append(data)
        elif kind == b"IEND":
            ended = True
        pos += 12 + n
    if head is None or not ended:
        raise ValueError(f"{path}: no IHDR or no IEND")
    W, H, bits, colour, comp, filt, lace = head
    if (bits, colour, comp, filt, lace) != (16, 0, 0, 0, 0):
        raise ValueError(f"{path}: expected 16-bit greyscale, not interlaced")
    flat = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    stride = 2 * W
    if flat.size != H * (1 + stride):
        raise ValueError(f"{path}: wrong amount of image data")
    rows = flat.reshape(H, 1 + stride)
    out = np.zeros((H, stride), np.uint8)
    prev = np.zeros(stride, np.uint8)
    for y in range(H):
        ft, line = int(rows[y, 0]), rows[y, 1:]
        if ft == 0:
            cur = line.copy()
        elif ft == 2:
            cur = line + prev
        elif ft in (1, 3, 4):  # these depend on the pixel to the left (two bytes back)
            cur = np.zeros(stride, np.uint8)
            for x in range(stride):
                left = cur[x - 2] if x >= 2 else np.uint8(0)
                ul = prev[x - 2] if x >= 2 else np.uint8(0)
                if ft == 1:
                    p = int(left)
                elif ft == 3:
                    p = (int(left) + int(prev[x])) >> 1
                else:
                    p = int(_paeth(np.array([left]), np.array([prev[x]]), np.array([ul]))[0])
                cur[x] = (int(line[x]) + p) & 0xFF
        else:
            raise ValueError(f"{path}: unknown row filter {ft}")
        out[y] = cur
        prev = cur
    return out.view(">u2").astype(np.uint16).reshape(H, W)


# ---- the encode ----------------------------------------------------------------------------------------

@dataclass
class DepthMaps:
    """u16: (K, H, W) the normalised inverse depth maps as the PNGs hold them (int32 on the device:
    torch has little arithmetic on uint16; values 0 .. 65535); scale, offset: (K,) float64 arrays, the
    entries of depth_params.json."""
    u16: torch.Tensor
    scale: np.ndarray
    offset: np.ndarray

    def invdepth(self) -> List[Optional[torch.Tensor]]:
        """Per image the (1, H, W) float32 supervision map of scene/cameras.py:72-74 -- the PNG read
        as u16 / 65536 (the reader's 2^16 against the writer's 65535 is the reference's), times scale
        plus offset, negatives set to 0 -- or None where scale <= 0 (the reference has no depth for
        such a view).  The reader's resize is not applied."""
        out = []
        for k in range(self.u16.shape[0]):
            if not self.scale[k] > 0:
                out.append(None)
                continue
            # cv2.imread(...).astype(np.float32) / float(2 ** 16), then float32 * python float + python float
            m = self.u16[k].to(torch.float32) / 65536.0
            m = m * float(self.scale[k]) + float(self.offset[k])
            out.append(torch.clamp_min(m, 0.0)[None])
        return out

    def depth_mask(self) -> List[Optional[torch.Tensor]]:
        """Per image invdepth > 0 as float32 (1, H, W), None where invdepth() is."""
        return [None if m is None else (m > 0).to(torch.float32) for m in self.invdepth()]

    def save(self, directory, names) -> None:
        """Write image k as directory/names[k] with its extension replaced by .png (16-bit greyscale);
        subdirectories in a name (cam0/...) are created."""
        names = list(names)
        if len(names) != self.u16.shape[0]:
            raise ValueError("names: expected one per image")
        host = self.u16.detach().cpu().numpy().astype(np.uint16)
        for k, name in enumerate(names):
            path = os.path.join(directory, os.path.splitext(name)[0] + ".png")
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            save_png16(path, host[k])


def encode_depth_maps(distance: torch.Tensor, quantize: bool = True, min_depth: float = 0.1,
                      max_depth: Optional[float] = None) -> DepthMaps:
    """distance: (K, H, W) float32 on the device, 0 where there is no surface (render_mesh_distance's
    output).  quantize: pass the distances through the reference's 3-channel code first (4, 16 and
    64 mm steps up to 65.536, 262.144 and 1048.576 m), as its pipeline does between the ray cast and
    this step.  Valid pixels are those with min_depth < depth (< max_depth)."""
    require_gpu(distance)
    if distance.dim() != 3 or distance.dtype != torch.float32:
        raise ValueError("distance: expected (K, H, W) float32")
    min_depth = float(min_depth)
    if not (min_depth >= 0.0 and np.isfinite(min_depth)):
        raise ValueError("min_depth: expected a finite value >= 0")
    md = 0.0 if max_depth is None else float(max_depth)
    if max_depth is not None and not md > 0.0:
        raise ValueError("max_depth: expected None or a value > 0")
    distance = distance.detach().contiguous()
    K, H, W = distance.shape
    dev = distance.device
    u16 = torch.zeros((K, H, W), dtype=torch.int32, device=dev)
    scale, offset = np.zeros(K, np.float64), np.zeros(K, np.float64)
    if K == 0 or H == 0 or W == 0:
        return DepthMaps(u16, scale, offset)
    L = lib()
    with torch.cuda.device(dev):
        for k0 in range(0, K, 65535):
            n = min(65535, K - k0)
            raw = torch.empty((n, H, W), dtype=torch.int16, device=dev)  # the uint16 bits
            scratch = torch.empty(L.gsr_depth_encode_scratch_bytes(n), dtype=torch.uint8, device=dev)
            s, o = (ctypes.c_double * n)(), (ctypes.c_double * n)()
            check(L.gsr_depth_encode(n, H, W, ptr(distance[k0:k0 + n]), 1 if quantize else 0, min_depth, md,
                                     ptr(scratch), ptr(raw), s, o, stream(dev)), "gsr_depth_encode")
            u16[k0:k0 + n] = raw.to(torch.int32) & 0xFFFF
            scale[k0:k0 + n], offset[k0:k0 + n] = np.frombuffer(s, np.float64), np.frombuffer(o, np.float64)
    return DepthMaps(u16, scale, offset)


# ---- depth_params.json ---------------------------------------------------------------------------------

def write_depth_params(path, names, maps, default_scale: float = 0.0, default_offset: float = 0.0) -> int:
    """depth_params.json as write_depth_params_for_model leaves it (depth_map_to_distances.py:419-504):
    one entry per name of `names` (a model's image names), keyed without extension, sorted, indent 4;
    `maps` is {name without extension: (scale, offset)} -- or a (names, DepthMaps) pair -- and a name
    with no map gets the defaults.  Returns the number of entries."""
    if isinstance(maps, tuple) and len(maps) == 2 and isinstance(maps[1], DepthMaps):
        mnames, m = maps
        maps = {os.path.splitext(n)[0]: (float(m.scale[k]), float(m.offset[k])) for k, n in enumerate(mnames)}
    out = {}
    for n in names:
        base = os.path.splitext(n)[0]
        so = maps.get(base)
        out[base] = {"scale": float(so[0]), "offset": float(so[1])} if so is not None else \
            {"scale": default_scale, "offset": default_offset}
    out = dict(sorted(out.items(), key=lambda kv: kv[0]))
    with open(path, "w") as f:
        json.dump(out, f, indent=4)
    return len(out)


def read_depth_params(path) -> dict:
    """The file's entries with med_scale added to each, as scene/dataset_readers.py:264-279 does: the
    median of the scales > 0, or 0 when there is none."""
    with open(path, "r") as f:
        params = json.load(f)
    scales = np.array([params[k]["scale"] for k in params], dtype=np.float64)
    med = float(np.median(scales[scales > 0])) if (scales > 0).sum() else 0
    for k in params:
        params[k]["med_scale"] = med
    return params
