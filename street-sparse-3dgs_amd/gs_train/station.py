"""Station render: the cube faces of one recording position from one hierarchy cut
(include/gsr_station.h, csrc/station.hip).  Inference only.

A street recording is a set of stations: one camera centre with four to six faces around it
(render_position.py groups its cameras by centre).  The reference's render scripts draw every
camera on its own: expand_to_size, get_interpolation_weights and render_post per camera.  The cut,
the weights, the child / parent blend, the world-space covariance and the SH colour read the centre
only, so here they run once per station:

    stations = group_stations([c.camera_center for c in cameras])
    sr = StationRenderer(model, "cuda")
    for idx in stations:
        images, invdepths, radii = sr.render([cameras[i] for i in idx], tau)
        for k, i in enumerate(idx):
            evaluator.add_view({"render": images[k], "depth": invdepths[k]}, cameras[i])

Limits: no backward; the faces of a call share width, height and field of view (so that the cut's
threshold is one value); one centre; M = 16 SH coefficients per row.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from diff_gaussian_rasterization import _lib
from ._native import check, lib, ptr, stream
from .synthetic import tau_threshold

MAX_FACES = _lib.STATION_MAX_FACES


def group_stations(centers, tol: float = 0.0, decimals=None):
    """Lists of camera indices that share a centre, in order of first appearance, each list in camera
    order.  Default: only bitwise-equal centres (as float32 triples) share a station.  decimals=d: the
    key is tuple(np.round(center, d)); d = 2 is render_position.py's key.  tol > 0: a camera joins the
    first station whose first member's centre lies within `tol` (Euclidean) of its own.  Pure host
    code; `centers` is a sequence of 3-vectors (arrays, lists or tensors)."""
    cs = [np.asarray(c.detach().cpu().numpy() if hasattr(c, "detach") else c, dtype=np.float32).reshape(3)
          for c in centers]
    if decimals is not None and tol:
        raise ValueError("group_stations: give decimals or tol, not both")
    groups: list[list[int]] = []
    if tol:
        if tol < 0:
            raise ValueError("group_stations: tol must be >= 0")
        firsts = []
        for i, c in enumerate(cs):
            for g, f in enumerate(firsts):
                if float(np.linalg.norm(c.astype(np.float64) - f.astype(np.float64))) <= tol:
                    groups[g].append(i)
                    break
            else:
                firsts.append(c)
                groups.append([i])
        return groups
    seen: dict = {}
    for i, c in enumerate(cs):
        key = tuple(np.round(c, decimals=decimals)) if decimals is not None else c.tobytes()
        if key not in seen:
            seen[key] = len(groups)
            groups.append([])
        groups[seen[key]].append(i)
    return groups


def _get(o, *names):
    for n in names:
        if isinstance(o, dict):
            if n in o:
                return o[n]
        elif hasattr(o, n):
            return getattr(o, n)
    raise KeyError(f"camera / model has none of {names}")


def _camera(c):
    """(view (16,), proj (16,), campos (3,), tanfovx, tanfovy, W, H) of a dict (gs_train.synthetic's
    keys) or of a reference Camera (scene/cameras.py's attributes)."""
    f32 = lambda a: (a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)).astype(np.float32).reshape(-1)
    view = f32(_get(c, "view", "world_view_transform"))
    proj = f32(_get(c, "proj", "full_proj_transform"))
    campos = f32(_get(c, "campos", "camera_center"))
    try:
        tx, ty = float(_get(c, "tanfovx")), float(_get(c, "tanfovy"))
    except KeyError:
        tx, ty = math.tan(float(_get(c, "FoVx")) * 0.5), math.tan(float(_get(c, "FoVy")) * 0.5)
    return view, proj, campos, tx, ty, int(_get(c, "W", "image_width")), int(_get(c, "H", "image_height"))


class _Grow:
    """A grow-only device byte buffer behind a gsr_resize_fn."""

    def __init__(self, device):
        self.device = device
        self.t = None
        self.fn = _lib.RESIZE_FN(self._resize)

    def _resize(self, _ctx, nbytes):
        try:
            if self.t is None or self.t.numel() < nbytes:
                self.t = None
                self.t = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=self.device)
            return self.t.data_ptr()
        except Exception:  # the C side reports GSR_ERR_ALLOCATION
            return 0


class StationRenderer:
    """render(cameras, tau) draws the faces of one station from one cut of the hierarchy.

    model_or_tensors: a dict with means3D (N,3), scales (N,3), rotations (N,4), opacities (N,1),
    shs (N,16,3) -- activated, as render_post reads them --, nodes (Nn,7) int32, boxes (Nn,2,4) and
    skybox (the S last rows; gs_train.synthetic.synthetic_lod_hierarchy's keys), or an object with the
    reference model's get_xyz / get_scaling / get_rotation / get_opacity / get_features, nodes, boxes
    and skybox_points.  The tensors are read at every call (no copy is kept when they already are
    contiguous float32 on the device).  The scratch, the compact rows and the frame buffers are kept
    between calls and only grow; they carry no state from one call to the next."""

    def __init__(self, model_or_tensors, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("StationRenderer needs a ROCm GPU device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.model = model_or_tensors
        self._geom, self._bin, self._img, self._rows = (_Grow(self.device) for _ in range(4))
        self._scratch = None
        self._cut = None  # ri, pi, ni, w, kids: N_nodes + S entries
        self.last_kept = None   # rows each face kept (list of int)
        self.last_K = None      # tile instances per face
        self.last_cut = None    # (render_indices, parent_indices, weights) views of the last call, R rows
        self._last_offsets = None

    # -- the model's tensors ------------------------------------------------------------------
    def _tensors(self):
        m = self.model
        t = lambda x: x.detach().to(device=self.device, dtype=torch.float32).contiguous()
        means = t(_get(m, "means3D", "get_xyz"))
        scales = t(_get(m, "scales", "get_scaling"))
        rots = t(_get(m, "rotations", "get_rotation"))
        opac = t(_get(m, "opacities", "get_opacity")).reshape(-1)
        shs = t(_get(m, "shs", "get_features"))
        if shs.dim() != 3 or shs.shape[1] != 16 or shs.shape[2] != 3:
            raise ValueError(f"StationRenderer needs shs of shape (N, 16, 3), got {tuple(shs.shape)}")
        N = means.shape[0]
        if not (scales.shape[0] == rots.shape[0] == opac.shape[0] == shs.shape[0] == N):
            raise ValueError("StationRenderer: the model's tensors differ in row count")
        return means, scales, rots, opac, shs

    def _hier(self):
        m = self.model
        nodes = _get(m, "nodes").to(device=self.device, dtype=torch.int32).contiguous()
        boxes = _get(m, "boxes").to(device=self.device, dtype=torch.float32).contiguous()
        return nodes, boxes, int(_get(m, "skybox", "skybox_points"))

    # -- one station ---------------------------------------------------------------------------
    def render(self, cameras, tau, center=None, bg=(0.0, 0.0, 0.0), do_depth=True, sh_degree=3):
        """(images (F,3,H,W), invdepths (F,1,H,W) or None, radii (F,R) int32) of the F cameras.

        The cameras must share W, H and tanfov (the cut's threshold is then one value,
        render_hierarchy.py:61).  expand_to_size and get_interpolation_weights run once, at `center`
        (default: the first camera's centre); the skybox rows are appended to the cut with weight 1 and
        themselves as parent.  radii[f] holds face f's radii at the rows' places in the cut (the cut's
        R rows, skybox rows last), zero for rows the face does not draw.

        When the cameras' centres are not bitwise equal, every face is still drawn with the cut and
        the SH directions of `center`: the faces' own view matrices project rows whose level of
        detail and colour were chosen for `center`.  That is an approximation, not the per-camera
        result, and it is the caller's choice (group_stations' decimals / tol)."""
        from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
        cams = [_camera(c) for c in cameras]
        if not cams:
            raise ValueError("StationRenderer.render: no cameras")
        W, H, tx = cams[0][5], cams[0][6], cams[0][3]
        ctr = cams[0][2] if center is None else np.asarray(
            center.detach().cpu().numpy() if hasattr(center, "detach") else center, np.float32).reshape(3)
        nodes, boxes, S = self._hier()
        Nn = nodes.shape[0]
        N = int(_get(self.model, "means3D", "get_xyz").shape[0])
        cap = max(N, Nn + S)  # a node can hold several Gaussians: the cut has at most N - S entries
        if self._cut is None or self._cut[0].numel() < cap:
            i32 = lambda: torch.zeros(cap, dtype=torch.int32, device=self.device)
            self._cut = (i32(), i32(), i32(), torch.zeros(cap, device=self.device), i32())
        ri, pi, ni, w, kids = self._cut
        thr = float(np.float32(tau_threshold(tau, tx, W)))
        vp = torch.tensor(ctr, device=self.device)
        n = expand_to_size(nodes, boxes, thr, vp, torch.zeros(3), ri[:cap - S], pi[:cap - S], ni[:cap - S])
        get_interpolation_weights(ni[:n], thr, nodes, boxes, vp.cpu(), torch.zeros(3), w, kids)
        if S:
            sky = torch.arange(N - S, N, dtype=torch.int32, device=self.device)
            ri[n:n + S] = sky
            pi[n:n + S] = sky
            w[n:n + S] = 1.0
        R = n + S
        return self.render_cut(cameras, ri[:R], pi[:R], w[:R], center=ctr, bg=bg, do_depth=do_depth,
                               sh_degree=sh_degree)

    def render_cut(self, cameras, render_indices, parent_indices, weights, center=None, bg=(0.0, 0.0, 0.0),
                   do_depth=True, sh_degree=3):
        """render() from a cut the caller made: R device entries each of render_indices /
        parent_indices (int32; parent -1 = the last row) and weights (float32)."""
        cams = [_camera(c) for c in cameras]
        F = len(cams)
        if F < 1:
            raise ValueError("StationRenderer.render: no cameras")
        W, H, tx, ty = cams[0][5], cams[0][6], cams[0][3], cams[0][4]
        for c in cams[1:]:
            if (c[5], c[6]) != (W, H) or c[3] != tx or c[4] != ty:
                raise ValueError("StationRenderer.render: the cameras of a station must share W, H and tanfov")
        dev = self.device
        ctr = cams[0][2] if center is None else np.asarray(
            center.detach().cpu().numpy() if hasattr(center, "detach") else center, np.float32).reshape(3)
        means, scales, rots, opac, shs = self._tensors()
        N = means.shape[0]
        ri = render_indices.to(device=dev, dtype=torch.int32).contiguous()
        R = int(ri.shape[0])
        if parent_indices.shape[0] < R or weights.shape[0] < R:
            raise ValueError("parent_indices / weights shorter than render_indices")
        pi = parent_indices[:R].to(device=dev, dtype=torch.int32).contiguous()
        w = weights[:R].detach().to(device=dev, dtype=torch.float32).contiguous()
        views = torch.tensor(np.stack([c[0] for c in cams]), device=dev)
        projs = torch.tensor(np.stack([c[1] for c in cams]), device=dev)
        campos = torch.tensor(ctr, device=dev)
        bg_t = torch.as_tensor(bg, dtype=torch.float32).reshape(3).to(dev)
        L = lib()
        need = int(L.gsr_station_rows_scratch_bytes(R, F)) if F <= MAX_FACES else 0
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = None
            self._scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        images = torch.empty(F, 3, H, W, device=dev)
        invd = torch.empty(F, 1, H, W, device=dev) if do_depth else None
        radii = torch.empty(F, R, dtype=torch.int32, device=dev)
        K = (ctypes.c_int64 * max(F, 1))()
        kept = (ctypes.c_int64 * max(F, 1))()
        with torch.cuda.device(dev):
            rc = L.gsr_rasterize_station_forward(
                self._geom.fn, self._bin.fn, self._img.fn, self._rows.fn, None, ptr(self._scratch),
                self._scratch.numel(), N, int(sh_degree), int(shs.shape[1]), ptr(means), ptr(shs), ptr(opac),
                ptr(scales), ptr(rots), ptr(ri), ptr(pi), ptr(w), R, F, ptr(views), ptr(projs), ptr(campos),
                float(tx), float(ty), W, H, ptr(bg_t), ptr(images), ptr(invd), ptr(radii), K, kept, 0, stream(dev))
        check(rc, "gsr_rasterize_station_forward")
        self.last_K = [int(K[f]) for f in range(F)]
        self.last_kept = [int(kept[f]) for f in range(F)]
        self.last_cut = (ri, pi, w)
        offs = (ctypes.c_size_t * (F * _lib.STATION_FACE_ARRAYS))()
        L.gsr_station_rows_layout(F, kept, offs)
        self._last_offsets = [int(o) for o in offs]
        return images, invd, radii

    def face_rows(self, f):
        """Face f's compact rows of the last call, as views of the kept buffer (valid until the next
        call): dict(means (P,3), cov3D (P,6), opacity (P,), rgb (P,3), src (P,) int32 = the row's
        index in the cut)."""
        P = self.last_kept[f]
        o = self._last_offsets[f * _lib.STATION_FACE_ARRAYS:(f + 1) * _lib.STATION_FACE_ARRAYS]
        buf = self._rows.t
        if P == 0 or buf is None:
            e = lambda *s: torch.empty(*s, device=self.device)
            return dict(means=e(0, 3), cov3D=e(0, 6), opacity=e(0), rgb=e(0, 3),
                        src=torch.empty(0, dtype=torch.int32, device=self.device))
        fl = lambda off, width: buf[off:off + 4 * width * P].view(torch.float32).view(P, width)
        return dict(means=fl(o[0], 3), cov3D=fl(o[1], 6), opacity=fl(o[2], 1).view(P), rgb=fl(o[3], 3),
                    src=buf[o[4]:o[4] + 4 * P].view(torch.int32))


def set_profiling(enable: bool) -> bool:
    """Record HIP events around the stages of the station calls (gsr_station_set_profiling)."""
    return bool(lib().gsr_station_set_profiling(int(bool(enable))))


STAGES = ("station_rows", "counts_and_compact", "face_frames", "radii_scatter")


def stage_times_ms() -> dict:
    """Device milliseconds of the last station call's stages on this thread (after set_profiling(True))."""
    buf = (ctypes.c_float * len(STAGES))()
    n = lib().gsr_station_stage_times_ms(buf, len(STAGES))
    return {STAGES[i]: float(buf[i]) for i in range(n)}
