"""NativePostStep: PostTrainStep.step (post.py) as ONE native call, gsr_post_step
(include/gsr_post.h, csrc/post_step.hip).

The host keeps train_post.py's schedule arithmetic -- the random LOD limit drawn from the host
generator (:73-74), the xyz learning rate, Adam's step counts and bias corrections in double -- and
hands the iteration to the executor, which issues the entry points PostTrainStep reaches through
autograd in the same order and ends in gsr_post_adam_step: the locked rows' zeroing, the Adam update
and the gradients' clear in one launch that walks only the rows this cut touched and the rows whose
moments are still nonzero.

The parameters and the Adam moments (the optimizer's own state tensors, so checkpoint code sees
them) stay the Python objects'.  `.grad` stays None; the gradients live in `self.grads`, five N-row
buffers that are all zero between iterations.  The set-up is redone whenever the parameter or moment
tensors are replaced (a checkpoint restore), which also rebuilds the executor's live-row table
from the moments.
"""
from __future__ import annotations

import ctypes
import math

import torch

from diff_gaussian_rasterization._lib import AdamGroup, PostStepArgs

from ._native import check, lib, require_gpu, stream
from .post import PostTrainStep

_PARAMS = ("_xyz", "_features", "_opacity", "_scaling", "_rotation")
_FIELDS = ("xyz", "features", "opacity", "scaling", "rotation")


class NativePostStep(PostTrainStep):
    def __init__(self, *args, **kw):
        self._ctx = None
        super().__init__(*args, **kw)
        self._key = None
        self.grads = None
        # step() cuts inside the executor: the Python cut's five N-entry buffers are made when cut() is
        # first called (synthetic_post_problem's targets, a reference step built on this one)
        self.ri = self.pi = self.ni = self.w = self.kids = None
        ctx = lib().gsr_post_ctx_create()
        if not ctx:
            raise RuntimeError("gsr_post_ctx_create failed")
        self._ctx = ctypes.c_void_p(ctx)

    def __del__(self):
        ctx = getattr(self, "_ctx", None)
        if ctx is not None and ctx.value:
            try:
                lib().gsr_post_ctx_destroy(ctx)
            except Exception:  # interpreter shutdown
                pass
            self._ctx = None

    def cut(self, k, limit):
        if self.ri is None:
            Nn, dev = self.m.N, self.m._xyz.device
            self.ri, self.pi, self.ni, self.kids = (torch.zeros(Nn, dtype=torch.int32, device=dev) for _ in range(4))
            self.w = torch.zeros(Nn, dtype=torch.float32, device=dev)
        return super().cut(k, limit)

    def ctx_stats(self) -> dict:
        """The executor's grow-only buffers: growths since creation, bytes held, stream-ordered
        growth (gsr_post_ctx_stats)."""
        buf = (ctypes.c_int64 * 3)()
        lib().gsr_post_ctx_stats(self._ctx, buf, 3)
        return {"growths": int(buf[0]), "bytes": int(buf[1]), "stream_ordered": bool(buf[2])}

    def row_state(self):
        """(live (N) uint8, stamp (N) int32, the last stamp value) after the last step: live = the
        row's moments may be nonzero, stamp = the value of the last step that touched the row (0:
        no step has)."""
        N, dev = self.m.N, self.m._xyz.device
        live = torch.empty(N, dtype=torch.uint8, device=dev)
        stamp = torch.empty(N, dtype=torch.int32, device=dev)
        cur = ctypes.c_int(0)
        with torch.cuda.device(dev):
            check(lib().gsr_post_ctx_read_rows(self._ctx, 0, live.data_ptr(), N, ctypes.byref(cur)), "gsr_post_ctx_read_rows")
            check(lib().gsr_post_ctx_read_rows(self._ctx, 1, stamp.data_ptr(), N, None), "gsr_post_ctx_read_rows")
        return live, stamp, cur.value

    # ---- set-up (again whenever the parameter or moment tensors are replaced) ----
    def _state(self, p):
        st = self.optimizer.state[p]
        if len(st) == 0:  # Adam.step's lazy initialisation
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _params_key(self):
        m = self.m
        moments = tuple(
            (id(st), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()) if "exp_avg" in st else (id(st),)
            for group in self.optimizer.param_groups for p in group["params"]
            for st in (self.optimizer.state.get(p, {}),))
        return tuple((getattr(m, n).data_ptr(), tuple(getattr(m, n).shape)) for n in _PARAMS) + \
            (m.nodes.data_ptr(), m.boxes.data_ptr(), m.anchors.data_ptr(), m.anchors.numel(), m.skybox_points) + moments

    def _setup(self):
        m = self.m
        require_gpu(m._xyz)
        for n in _PARAMS:
            t = getattr(m, n)
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{n}: the native step needs contiguous float32 parameters")
        dev = m._xyz.device
        self.grads = {n: torch.zeros_like(getattr(m, n)) for n in _PARAMS}
        by_id = {id(getattr(m, n)): self.grads[n] for n in _PARAMS}
        self._entries = []
        for group in self.optimizer.param_groups:
            for p in group["params"]:
                st = self._state(p)
                if not (st["exp_avg"].is_contiguous() and st["exp_avg_sq"].is_contiguous()):
                    raise ValueError("the native step needs contiguous moment buffers")
                row = p.numel() // max(p.shape[0], 1)
                for start, stop, _ in group.get("column_lrs", [(None, None, None)]):
                    start, stop = (0, row) if start is None else (start, stop)
                    off = 4 * start
                    self._entries.append((group, p, st, start, AdamGroup(
                        p.data_ptr() + off, by_id[id(p)].data_ptr() + off, st["exp_avg"].data_ptr() + off,
                        st["exp_avg_sq"].data_ptr() + off, stop - start, 0.0, 0.0, row)))
        b = {tuple(gr["betas"]) + (gr["eps"],) for gr in self.optimizer.param_groups}
        if len(b) != 1:
            raise NotImplementedError("the native step needs the same betas / eps in every group")
        (b1, b2, eps), = b
        self._groups = (AdamGroup * len(self._entries))(*[e[4] for e in self._entries])
        # the anchors as one byte per row (train_post.py:176-181 indexes the gradients with them)
        self._lock = None
        if m.anchors.numel():
            self._lock = torch.zeros(m.N, dtype=torch.uint8, device=dev)
            self._lock[m.anchors.to(dev).long()] = 1
        a = PostStepArgs()
        a.N, a.n_nodes, a.M, a.skybox = m.N, m.nodes.shape[0], m._features.shape[1], m.skybox_points
        a.width, a.height = self.W, self.H
        a.nodes, a.boxes = m.nodes.data_ptr(), m.boxes.data_ptr()
        for n, f in zip(_PARAMS, _FIELDS):
            setattr(a, f, getattr(m, n).data_ptr())
            setattr(a, f + "_grad", self.grads[n].data_ptr())
        a.n_groups = len(self._entries)
        a.groups = self._groups
        a.beta1, a.beta2, a.eps = b1, b2, eps
        a.lock = self._lock.data_ptr() if self._lock is not None else None
        a.background = self.bg.data_ptr()
        a.lambda_dssim = self.lambda_dssim
        self._args = a
        self._rebuild = True  # the executor's live rows come from these moments
        self._key = self._params_key()

    def _advance(self):
        """Adam.step's bookkeeping: one step per parameter, bias corrections in double."""
        seen = {}
        for i, (group, p, st, start, _grp) in enumerate(self._entries):
            if id(p) not in seen:
                st["step"] += 1
                seen[id(p)] = st["step"].item()
            s = seen[id(p)]
            b1, b2 = group["betas"]
            lr = group["lr"]
            if "column_lrs" in group:
                lr = next(l for a0, _a1, l in group["column_lrs"] if a0 == start)
            self._groups[i].step_size = lr / (1 - b1 ** s)
            self._groups[i].bias_correction2_sqrt = math.sqrt(1 - b2 ** s)

    def step(self, cam_idx=None):
        m = self.m
        if self._key is None or self._key != self._params_key():
            self._setup()
        it = self.iteration
        k = (it - 1) % len(self.cams) if cam_idx is None else cam_idx
        limit = self._limit()
        for pg in self.optimizer.param_groups:
            if pg["name"] == "xyz":
                pg["lr"] = self.xyz_lr(it)
        if it % 1000 == 0 and m.active_sh_degree < m.max_sh_degree:  # :88-89
            m.active_sh_degree += 1
        self._advance()
        dev = m._xyz.device
        c = self.cams[k]
        a = self._args
        a.D = m.active_sh_degree
        a.rebuild_live = int(self._rebuild)
        a.viewmatrix, a.projmatrix, a.campos = c["view"].data_ptr(), c["proj"].data_ptr(), c["campos"].data_ptr()
        for j, v in enumerate(c["campos_cpu"].detach().reshape(3).tolist()):
            a.campos_host[j] = float(v)
        a.tan_fovx, a.tan_fovy = c["tx"], c["ty"]
        a.limit = float(limit)
        a.gt = self.gts[k].data_ptr()
        am, E = self.amask[k], self.expo[k]
        for name, t in (("gt", self.gts[k]), ("alpha_mask", am), ("exposure", E)):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev):
                raise ValueError(f"{name}: the native step needs contiguous float32 tensors on the model's device")
        a.alpha_mask = am.data_ptr() if am is not None else None
        a.exposure = E.data_ptr() if E is not None else None
        losses = torch.empty(3, dtype=torch.float32, device=dev)  # a fresh tensor per step
        a.losses = losses.data_ptr()
        a.stream = stream(dev).value
        R, K = ctypes.c_int64(0), ctypes.c_int64(0)
        with torch.cuda.device(dev):
            rc = lib().gsr_post_step(self._ctx, ctypes.byref(a), ctypes.byref(R), ctypes.byref(K))
        if rc != 0:
            # a step that failed after the blend's backward may have left gradient rows behind: the next
            # step's set-up zeroes the gradients again and rebuilds the live rows from the moments
            self._key = None
            check(rc, "gsr_post_step")
        self._rebuild = False
        self.last_cut = R.value
        self.last_K = K.value
        self.iteration += 1
        return losses[2]
