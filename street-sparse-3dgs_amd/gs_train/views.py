"""A chunk's training views, compact and resident on the device (include/gsr_views.h, csrc/views.hip).

Replaces, between a decoded image and the step, the reference's utils/camera_utils.py:22-92 (loadCam),
utils/general_utils.py:22-29 (PILtoTorch) and scene/cameras.py:47-88 (Camera.__init__): the Lanczos
resize to the training resolution, the alpha mask, the 16-bit inverse depth map with its scale and
offset, the train_test_exp half mask.  The reference makes a view's float32 planes on DataLoader
workers once per iteration; the native step takes under a millisecond, so here a chunk's views stay
on the device as they sit in their files -- RGB8, mask8, depth16: a quarter of the float32 planes --
and a view's planes are rebuilt, bit for bit, by one streaming kernel each time the view comes up.

File decoding (JPEG / PNG), RGBA images and camera_to_JSON stay with the caller."""
from __future__ import annotations

import ctypes
from fractions import Fraction
from typing import Optional

import numpy as np
import torch

from ._native import check, lib, ptr, require_gpu, stream


def target_resolution(orig_w: int, orig_h: int, resolution=-1, resolution_scale: float = 1.0,
                      reference_floats: bool = False):
    """(width, height) of loadCam:64-81.  resolution 1, 2, 4, 8: each side divided by
    resolution_scale * resolution and rounded with Python's round (ties to even).  -1: images wider
    than 1600 are scaled to a width of 1600, int() truncating.  Any other value: the target width.

    The rule is evaluated exactly (the arguments as the rationals they are), so a capped image is 1600
    wide: 1601 x 1200 gives (1600, 1199).  reference_floats=True evaluates it in Python's doubles,
    operation by operation as loadCam does: there 1601 / (1601 / 1600) is 1599.9999999999998 and int()
    gives 1599 -- the reference trains 464 of the widths 1601 .. 7999 one pixel narrower than its cap.
    Pass it to reproduce a reference run's sizes to the pixel; the heights agree either way in those
    cases."""
    if reference_floats:
        w, h, res, rs = orig_w, orig_h, resolution, resolution_scale
    else:
        w, h, rs = Fraction(orig_w), Fraction(orig_h), Fraction(resolution_scale)
        res = resolution if resolution in (1, 2, 4, 8, -1) else Fraction(resolution)
    if resolution in (1, 2, 4, 8):
        return round(w / (rs * res)), round(h / (rs * res))
    if resolution == -1:
        global_down = w / 1600 if orig_w > 1600 else 1
    else:
        global_down = w / res
    scale = (float(global_down) * float(rs)) if reference_floats else global_down * rs
    return int(w / scale), int(h / scale)


class ResizePlan:
    """The coefficient tables of one resize geometry (gsr_resize_plan_create): made on the host when
    the plan is, uploaded by the first resize, reused by every later one."""

    def __init__(self, in_w: int, in_h: int, out_w: int, out_h: int):
        self._h = None
        self.in_w, self.in_h, self.out_w, self.out_h = int(in_w), int(in_h), int(out_w), int(out_h)
        h = lib().gsr_resize_plan_create(self.in_w, self.in_h, self.out_w, self.out_h)
        if not h:
            from diff_gaussian_rasterization import _lib
            raise ValueError(f"gsr_resize_plan_create failed: {_lib.last_error()}")
        self._h = ctypes.c_void_p(h)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                lib().gsr_resize_plan_destroy(h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    def info(self) -> dict:
        """uploads: table uploads so far; ksize_x, ksize_y: taps per output sample (0: pass skipped);
        table_bytes on the device; scratch_bytes per channel."""
        buf = (ctypes.c_int64 * 5)()
        check(lib().gsr_resize_plan_info(self._h, buf, 5), "gsr_resize_plan_info")
        return dict(zip(("uploads", "ksize_x", "ksize_y", "table_bytes", "scratch_bytes"), (int(v) for v in buf)))

    @property
    def uploads(self) -> int:
        return self.info()["uploads"]

    def tables(self, axis: int):
        """The host tables of axis 0 (horizontal) or 1 (vertical): (xmin[out], count[out],
        coeff[out, ksize]) int32 arrays."""
        n = self.out_w if axis == 0 else self.out_h
        ksize = self.info()["ksize_x" if axis == 0 else "ksize_y"]
        bounds, coeffs = np.zeros((n, 2), np.int32), np.zeros((n, max(ksize, 1)), np.int32)
        i32p = ctypes.POINTER(ctypes.c_int32)
        check(lib().gsr_resize_plan_tables(self._h, int(axis), bounds.ctypes.data_as(i32p), coeffs.ctypes.data_as(i32p)),
              "gsr_resize_plan_tables")
        return bounds[:, 0].copy(), bounds[:, 1].copy(), coeffs

    def resize(self, image: torch.Tensor) -> torch.Tensor:
        """image: (in_h, in_w) or (in_h, in_w, 3) uint8 on the device; returns (out_h, out_w[, 3])."""
        require_gpu(image)
        if image.dtype != torch.uint8 or image.dim() not in (2, 3) or tuple(image.shape[:2]) != (self.in_h, self.in_w):
            raise ValueError(f"image: expected ({self.in_h}, {self.in_w}[, 3]) uint8, got {tuple(image.shape)} {image.dtype}")
        C = 1 if image.dim() == 2 else int(image.shape[2])
        _check_channels(C)
        src = image.contiguous()
        dev = src.device
        L = lib()
        out = torch.empty((self.out_h, self.out_w) + tuple(image.shape[2:]), dtype=torch.uint8, device=dev)
        scratch = torch.empty(L.gsr_resize_scratch_bytes(self._h, C), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            check(L.gsr_resize_lanczos_u8(self._h, ptr(src), C, ptr(scratch), ptr(out), stream(dev)),
                  "gsr_resize_lanczos_u8")
        return out


def _check_channels(C: int) -> None:
    if C == 4:
        raise ValueError("a 4-channel image is refused: Pillow premultiplies an RGBA image's colour by its alpha "
                         "around the Lanczos filter, which a plain 4-channel pass does not reproduce; pass the RGB "
                         "image and the alpha plane as `mask`")
    if C not in (1, 3):
        raise ValueError(f"expected 1 or 3 interleaved channels, got {C}")


def _as_u8(name, a, device) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise ValueError(f"{name}: expected a uint8 array or tensor, got {getattr(t, 'dtype', type(t))}")
    return t.to(device).contiguous()


def resize_lanczos(image_u8, size, device="cuda", plan: Optional[ResizePlan] = None) -> torch.Tensor:
    """Image.resize(size, Image.LANCZOS) of an (H, W) or (H, W, 3) uint8 image, bit for bit, on the
    device.  size: (w, h).  A numpy image is moved to `device`; the result is a device tensor."""
    if isinstance(image_u8, torch.Tensor) and image_u8.is_cuda:
        device = image_u8.device
    if getattr(image_u8, "ndim", 0) == 3:
        _check_channels(int(image_u8.shape[2]))
    img = _as_u8("image", image_u8, torch.device(device))
    if img.dim() not in (2, 3):
        raise ValueError(f"image: expected (H, W) or (H, W, 3), got {tuple(img.shape)}")
    w, h = int(size[0]), int(size[1])
    if plan is None:
        plan = ResizePlan(img.shape[1], img.shape[0], w, h)
    elif (plan.in_w, plan.in_h, plan.out_w, plan.out_h) != (img.shape[1], img.shape[0], w, h):
        raise ValueError("plan: made for another geometry")
    return plan.resize(img)


class View:
    """What view(k) returns: the attributes the reference's loops and Evaluator.add_view read of a
    Camera.  The tensors are the store's plane set (valid as ViewStore documents)."""

    def __init__(self, planes: dict, width: int, height: int, depth_only: bool):
        self.original_image = planes["gts"]
        self.alpha_mask = planes["alpha_masks"]
        self.invdepthmap = planes["mono_invdepths"]
        self.depth_mask = planes["depth_masks"]
        self.depth_reliable = planes["mono_invdepths"] is not None
        self.image_width, self.image_height = width, height
        self.is_depth_only = depth_only


class _Planes:
    """One kind of plane of every view as a sequence (`__len__`, `__getitem__`): what the step
    constructors take in place of a list."""

    def __init__(self, store: "ViewStore", kind: str):
        self._store, self._kind = store, kind

    def __len__(self):
        return len(self._store)

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(len(self)))]
        return self._store._planes(k)[self._kind]

    def __iter__(self):
        return (self[k] for k in range(len(self)))


class ViewStore:
    """Training views kept compact on the device -- RGB8 and mask8 at the training resolution, the
    inverse depth as the source's 16 bits at the source's resolution -- with `slots` sets of float32
    planes that views are expanded into as they come up.

    gts, alpha_masks, mono_invdepths, depth_masks are sequences a TrainStep, NativeTrainStep,
    CoarseTrainStep or PostTrainStep takes in place of lists.  The first touch of view k expands all
    of its planes with one launch (gsr_view_expand) on the current stream, into the least recently
    used plane set; later touches of k return the same tensors without a launch.  Entries the
    reference's Camera would not have are None: the depth entries of a view with scale <= 0 or no
    depth map.  gts[k] of a depth-only view is the black image.

    A RETURNED TENSOR STAYS VALID UNTIL `slots` FURTHER DISTINCT VIEWS HAVE BEEN REQUESTED: the
    plane set is then reused, on the stream current at that request, and the tensor holds another
    view.  A step reads a view's planes in the call that asked for them, so slots=2 serves the step
    loops; hold planes across more views by cloning them."""

    def __init__(self, device="cuda", slots: int = 2):
        if int(slots) < 1:
            raise ValueError("slots: expected at least 1")
        self.device = torch.device(device)
        self._views = []
        self._slots = [dict(view=None, buf=None, planes=None, stamp=0) for _ in range(int(slots))]
        self._clock = 0
        self._plans = {}
        self.expansions = 0  # launches of gsr_view_expand so far
        self.gts = _Planes(self, "gts")
        self.alpha_masks = _Planes(self, "alpha_masks")
        self.mono_invdepths = _Planes(self, "mono_invdepths")
        self.depth_masks = _Planes(self, "depth_masks")

    def __len__(self):
        return len(self._views)

    @property
    def depth_only(self):
        """Per view, True for a depth-only view (the steps' depth_only argument)."""
        return [v["depth_only"] for v in self._views]

    # ---- filling the store ------------------------------------------------------------------------
    def _resized(self, name, a, resolution):
        t = _as_u8(name, a, self.device)
        if resolution is None or (t.shape[1], t.shape[0]) == tuple(resolution):
            return t
        key = (t.shape[1], t.shape[0], int(resolution[0]), int(resolution[1]))
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = ResizePlan(*key)
        return plan.resize(t)

    def _depth(self, invdepth_u16):
        if isinstance(invdepth_u16, torch.Tensor):
            if invdepth_u16.dtype.is_floating_point or invdepth_u16.dim() != 2:
                raise ValueError("invdepth_u16: expected a 2-D integer array with values 0 .. 65535")
            d = invdepth_u16.to(self.device)
            if d.numel() and (int(d.min()) < 0 or int(d.max()) > 65535):
                raise ValueError("invdepth_u16: values outside 0 .. 65535")
            return (d.to(torch.int32) & 0xFFFF).to(torch.int16).contiguous()  # the uint16 bits
        a = np.asarray(invdepth_u16)
        if a.ndim != 2 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("invdepth_u16: expected a 2-D integer array with values 0 .. 65535")
        if a.size and (int(a.min()) < 0 or int(a.max()) > 65535):
            raise ValueError("invdepth_u16: values outside 0 .. 65535")
        return torch.from_numpy(np.ascontiguousarray(a.astype(np.uint16).view(np.int16))).to(self.device)

    def add(self, image=None, mask=None, invdepth_u16=None, scale: float = 0.0, offset: float = 0.0, resolution=None,
            depth_only: bool = False, test_half: Optional[str] = None, depth_valid: str = "alpha") -> int:
        """Add a view; returns its index.

        image: (H, W, 3) uint8, numpy or torch (None for a depth-only view, whose image is black);
        mask: (H, W) uint8 or None; invdepth_u16: (dH, dW) integers 0 .. 65535 as the depth PNG holds
        them, or None, with the scale and offset of depth_params.json (the view has depth planes when
        scale > 0).  resolution: (w, h), e.g. target_resolution(...): image and mask are resized to
        it on the device as Image.resize(..., Image.LANCZOS) does; None keeps their size.  A
        depth-only view without a resolution has the size of its mask, else of its depth map.
        test_half: "left" or "right", the half of the alpha mask set to 0 (train_test_exp on a test
        view: scene/cameras.py:56-60 zeroes the left half in the test dataset, the right half in the
        train dataset).  depth_valid: "alpha": depth_mask = alpha_mask, the reference's;
        "alpha_and_hit": also 0 where the inverse depth is 0 (DepthMaps.depth_mask())."""
        if test_half not in (None, "left", "right"):
            raise ValueError("test_half: expected None, 'left' or 'right'")
        if depth_valid not in ("alpha", "alpha_and_hit"):
            raise ValueError("depth_valid: expected 'alpha' or 'alpha_and_hit'")
        if resolution is not None:
            resolution = (int(resolution[0]), int(resolution[1]))
            if min(resolution) < 1:
                raise ValueError("resolution: expected (w, h) >= 1")
        depth_only = bool(depth_only) or image is None
        rgb = None
        if not depth_only:
            if getattr(image, "ndim", 0) != 3:
                raise ValueError("image: expected (H, W, 3) uint8")
            _check_channels(int(image.shape[2]))
            if image.shape[2] != 3:
                raise ValueError("image: expected (H, W, 3) uint8")
            rgb = self._resized("image", image, resolution)
            resolution = (rgb.shape[1], rgb.shape[0])
        m8 = None
        if mask is not None:
            if getattr(mask, "ndim", 0) != 2 or str(mask.dtype).split(".")[-1] != "uint8":
                raise ValueError("mask: expected a single-channel (H, W) uint8 image, got "
                                 f"{tuple(getattr(mask, 'shape', ()))} {getattr(mask, 'dtype', type(mask))}")
            m8 = self._resized("mask", mask, resolution)
            resolution = resolution or (m8.shape[1], m8.shape[0])
        d16 = self._depth(invdepth_u16) if invdepth_u16 is not None else None
        if resolution is None:
            if d16 is None:
                raise ValueError("a view needs an image, a mask, a depth map or a resolution")
            resolution = (d16.shape[1], d16.shape[0])
        scale, offset = float(scale), float(offset)
        if not (np.isfinite(np.float32(scale)) and np.isfinite(np.float32(offset))):
            raise ValueError("scale, offset: expected finite float32 values")
        self._views.append(dict(rgb=rgb, mask=m8, depth=d16, scale=scale, offset=offset, size=resolution,
                                depth_only=depth_only, zero_half={None: 0, "left": 1, "right": 2}[test_half],
                                depth_valid=1 if depth_valid == "alpha_and_hit" else 0))
        return len(self._views) - 1

    def add_depth_maps(self, depth_maps, k0: int = 0) -> None:
        """Attach a mesh_depth.DepthMaps batch to views k0, k0 + 1, ...: image j's 16 bits, scale
        and offset become view k0 + j's depth map."""
        n = int(depth_maps.u16.shape[0])
        if k0 < 0 or k0 + n > len(self._views):
            raise ValueError(f"depth maps for views {k0} .. {k0 + n - 1}, the store has {len(self._views)}")
        for j in range(n):
            v = self._views[k0 + j]
            v["depth"] = self._depth(depth_maps.u16[j])
            v["scale"], v["offset"] = float(depth_maps.scale[j]), float(depth_maps.offset[j])
            for s in self._slots:  # planes made before the map was attached are stale
                if s["view"] == k0 + j:
                    s["view"], s["planes"] = None, None

    # ---- the planes -------------------------------------------------------------------------------
    @staticmethod
    def _has_depth(v) -> bool:
        return v["depth"] is not None and v["scale"] > 0

    @staticmethod
    def _plane_bytes(v) -> int:
        n = v["size"][0] * v["size"][1]
        pad = lambda b: (b + 15) // 16 * 16
        return pad(12 * n) + pad(4 * n) * (3 if ViewStore._has_depth(v) else 1)

    def _planes(self, k: int) -> dict:
        k = int(k)
        if k < 0:
            k += len(self._views)
        if not 0 <= k < len(self._views):
            raise IndexError(f"view {k} of {len(self._views)}")
        self._clock += 1
        for s in self._slots:
            if s["view"] == k:
                s["stamp"] = self._clock
                return s["planes"]
        s = min(self._slots, key=lambda s: s["stamp"])
        v = self._views[k]
        w, h = v["size"]
        n = w * h
        need = self._plane_bytes(v)
        if s["buf"] is None or s["buf"].numel() < need:
            s["buf"] = torch.empty(need, dtype=torch.uint8, device=self.device)
        pad = lambda b: (b + 15) // 16 * 16
        off = [0]

        def take(c):
            t = s["buf"][off[0]:off[0] + 4 * c * n].view(torch.float32).view(c, h, w)
            off[0] += pad(4 * c * n)
            return t

        image, alpha = take(3), take(1)
        depth = self._has_depth(v)
        invd, dmask = (take(1), take(1)) if depth else (None, None)
        d = v["depth"] if depth else None
        with torch.cuda.device(self.device):
            check(lib().gsr_view_expand(w, h, ptr(v["rgb"]), ptr(v["mask"]), v["zero_half"], ptr(d),
                                        d.shape[1] if depth else 0, d.shape[0] if depth else 0, v["scale"], v["offset"],
                                        v["depth_valid"], ptr(image), ptr(alpha), ptr(invd), ptr(dmask),
                                        stream(self.device)), "gsr_view_expand")
        self.expansions += 1
        s["view"], s["stamp"] = k, self._clock
        s["planes"] = dict(gts=image, alpha_masks=alpha, mono_invdepths=invd, depth_masks=dmask)
        return s["planes"]

    def view(self, k: int) -> View:
        """View k with original_image, alpha_mask, invdepthmap, depth_mask, depth_reliable,
        image_width, image_height and is_depth_only: what Evaluator.add_view and the reference's
        loops read.  Touches the view like the sequences do."""
        p = self._planes(k)
        v = self._views[int(k)]
        return View(p, v["size"][0], v["size"][1], v["depth_only"])

    def nbytes(self) -> dict:
        """compact: bytes of the stored views; planes: bytes of the `slots` plane sets, each sized
        for the largest view; expanded: what every view's float32 planes would take resident."""
        compact = sum(t.numel() * t.element_size() for v in self._views for t in (v["rgb"], v["mask"], v["depth"])
                      if t is not None)
        per_view = [self._plane_bytes(v) for v in self._views]
        return {"views": len(self._views), "compact": compact,
                "planes": len(self._slots) * max(per_view, default=0), "expanded": sum(per_view)}
