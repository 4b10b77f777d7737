"""build_hierarchy: the LOD hierarchy of a trained chunk on the device (include/gsr_hier_build.h,
csrc/hier_build.hip) -- the pipeline's GaussianHierarchyCreator step between train_single.py and
train_post.py (scripts/full_train.py:152,203-216):

    h = build_hierarchy(xyz, log_scales, rotations, opacities, shs, first_row=skybox_points)
    h.save(path)                      # the .hier file create_from_hier loads
    model = h.to_model(skybox_rows)   # or straight into gs_train.post.PostTrainStep

P Gaussians in, N = 2P - 1 nodes out, one Gaussian per node, in the layout expand_to_size,
get_interpolation_weights, HierarchyModel and write_hierarchy consume.  The rule (DESIGN.md
"Hierarchy builder") is this project's definition -- Kerbl et al. 2024 sec. 5 over an LBVH -- and is
parity-unpinned against the un-vendored gaussianhierarchy tool.  gs_train.hier_merge merges the
chunks' hierarchies into the scene's.  Not covered: anchors.bin, the compressed .hier variant, a PLY
front end.  There is no CPU path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from ._native import check, lib, ptr, require_gpu, stream

MAX_ROWS = 1 << 30


@dataclass
class Hierarchy:
    """N = 2P - 1 rows: means3D (N,3), log_scales (N,3), rotations (N,4) (a leaf's raw quaternion, an
    interior node's unit one), opacities (N,1) activated (an interior node's may exceed 1), shs
    (N,M,3), nodes (N,7) int32, boxes (N,2,4), leaf_rows (N) int32 (the input row of a leaf, -1 for an
    interior node), levels (the tree's depth + 1)."""
    means3D: torch.Tensor
    log_scales: torch.Tensor
    rotations: torch.Tensor
    opacities: torch.Tensor
    shs: torch.Tensor
    nodes: torch.Tensor
    boxes: torch.Tensor
    leaf_rows: torch.Tensor
    levels: int

    def _shs16(self, shs=None):
        shs = self.shs if shs is None else shs
        if shs.shape[1] == 16:
            return shs
        out = torch.zeros(shs.shape[0], 16, 3, dtype=shs.dtype, device=shs.device)  # create_from_hier's filler
        out[:, :shs.shape[1]] = shs
        return out

    def save(self, path):
        """The .hier file, as save_hier writes it (scene/gaussian_model.py:437-445): log-scales and
        activated opacities; SH padded with zeros to 16 coefficients."""
        from gaussian_hierarchy._C import write_hierarchy
        write_hierarchy(path, self.means3D, self._shs16(), self.opacities, self.log_scales, self.rotations, self.nodes,
                        self.boxes)

    def to_model(self, skybox_rows=None, **kw):
        """A gs_train.post.HierarchyModel of the hierarchy.  skybox_rows: (xyz, log_scales, rotations,
        opacities, shs) of the skybox Gaussians, activated opacities, appended after the N node rows
        as create_from_hier does (scene/gaussian_model.py:389-401)."""
        from .post import HierarchyModel
        cols = [self.means3D, self.log_scales, self.rotations, self.opacities, self._shs16()]
        S = 0
        if skybox_rows is not None:
            sky = [torch.as_tensor(t, dtype=torch.float32, device=self.means3D.device) for t in skybox_rows]
            S = sky[0].shape[0]
            sky[3] = sky[3].reshape(S, 1)
            sky[4] = self._shs16(sky[4].reshape(S, -1, 3))
            cols = [torch.cat([c, s.reshape((S,) + tuple(c.shape[1:]))]) for c, s in zip(cols, sky)]
        else:
            cols = [c.clone() for c in cols]  # the model's parameters are trained in place
        xyz, ls, rot, op, shs = cols
        kw.setdefault("device", self.means3D.device)
        return HierarchyModel(xyz, shs, op, torch.exp(ls), rot, self.nodes, self.boxes, skybox=S, **kw)


def build_hierarchy(xyz, log_scales, rotations, opacities, shs, first_row=0):
    """The hierarchy of rows [first_row, P) of a chunk's Gaussians (rows below first_row -- the skybox
    -- are left out of the tree; leaf_rows still name the caller's rows).  xyz (P,3) finite, log_scales
    (P,3), rotations (P,4) raw (r, x, y, z), opacities (P,1) or (P) activated, shs (P,M,3) with
    1 <= M <= 16: float32 tensors on one ROCm device.  One host read checks xyz, and the build reads
    one word per tree level."""
    tensors = (xyz, log_scales, rotations, opacities, shs)
    names = ("xyz", "log_scales", "rotations", "opacities", "shs")
    for t, n in zip(tensors, names):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"build_hierarchy: {n} must be a tensor")
    P0 = xyz.shape[0] if xyz.dim() == 2 else -1
    first_row = int(first_row)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("build_hierarchy: xyz must be (P, 3)")
    if tuple(log_scales.shape) != (P0, 3) or tuple(rotations.shape) != (P0, 4):
        raise ValueError("build_hierarchy: log_scales must be (P, 3) and rotations (P, 4)")
    if tuple(opacities.shape) not in ((P0, 1), (P0,)):
        raise ValueError("build_hierarchy: opacities must be (P, 1) or (P,)")
    if shs.dim() != 3 or shs.shape[0] != P0 or shs.shape[2] != 3 or not 1 <= shs.shape[1] <= 16:
        raise ValueError("build_hierarchy: shs must be (P, M, 3) with 1 <= M <= 16")
    if not 0 <= first_row < P0:
        raise ValueError("build_hierarchy: first_row must leave at least one row")
    if P0 - first_row > MAX_ROWS:
        raise ValueError("build_hierarchy: more than 2^30 rows")
    for t, n in zip(tensors, names):
        if t.dtype != torch.float32:
            raise ValueError(f"build_hierarchy: {n} must be float32")
    require_gpu(*tensors)
    dev = xyz.device
    if any(t.device != dev for t in tensors):
        raise RuntimeError("build_hierarchy: the inputs must be on one device")
    ins = [t.detach()[first_row:].contiguous() for t in tensors]
    if not bool(torch.isfinite(ins[0]).all()):
        raise ValueError("build_hierarchy: xyz has non-finite values")
    P, M = P0 - first_row, shs.shape[1]
    N = 2 * P - 1
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    out = [f(N, 3), f(N, 3), f(N, 4), f(N, 1), f(N, M, 3)]
    nodes = torch.empty(N, 7, dtype=torch.int32, device=dev)
    boxes = f(N, 2, 4)
    leaf_rows = torch.empty(N, dtype=torch.int32, device=dev)
    L = lib()
    scratch = torch.empty(int(L.gsr_hier_build_scratch_bytes(P)), dtype=torch.uint8, device=dev)
    levels = ctypes.c_int(0)
    with torch.cuda.device(dev):
        check(L.gsr_hier_build(P, M, *[ptr(t) for t in ins], *[ptr(t) for t in out], ptr(nodes), ptr(boxes),
                               ptr(leaf_rows), ctypes.byref(levels), ptr(scratch), scratch.numel(), stream(dev)),
              "gsr_hier_build")
    if first_row:
        leaf_rows = torch.where(leaf_rows >= 0, leaf_rows + first_row, leaf_rows)
    return Hierarchy(*out, nodes, boxes, leaf_rows, int(levels.value))


def stage_ms():
    """Device time of this thread's last build in ms: sort, topology, numbering, merge."""
    buf = (ctypes.c_float * 4)()
    n = lib().gsr_hier_build_stage_ms(buf, 4)
    return dict(zip(("sort", "topology", "numbering", "merge"), list(buf)[:n]))
