"""The post-optimisation stage around one iteration (post.PostTrainStep or
native_post.NativePostStep): what train_post.py does besides the iteration itself.

  load_hierarchy_model   create_from_hier (scene/gaussian_model.py:344-417): the .hier file, the
                         anchors.bin and exposure.json beside it, the scaffold's skybox rows
  save_hier              save_hier (:437-445): every row of the model, skybox rows included
  capture / restore      the checkpoint of a step (tensors only)
  TrainPost              train_post.py's loop (:69-198): the views in order, the SH schedule, the
                         stop at `iterations`, save and checkpoint callbacks
"""
from __future__ import annotations

import json
import os
import warnings

import numpy as np
import torch

from .post import HierarchyModel, PostTrainStep

ANCHORS_NAME = "anchors.bin"
EXPOSURE_NAME = "exposure.json"
_PARAMS = ("_xyz", "_features", "_opacity", "_scaling", "_rotation")


def read_anchors(path):
    """anchors.bin: a 4-byte count word, read and ignored as the reference ignores it (:354-356),
    then little-endian int32 rows to the end of the file.  int64 CPU tensor."""
    with open(path, "rb") as f:
        data = f.read()
    payload = data[4:]
    if len(data) < 4 or len(payload) % 4 != 0:
        raise ValueError(f"{path}: {len(data)} bytes are not a count word and whole int32 rows")
    return torch.from_numpy(np.frombuffer(payload, dtype="<i4").astype(np.int64))


def load_hierarchy_model(hier_path, scaffold_dir=None, spatial_lr_scale=1.0, device="cuda"):
    """create_from_hier: returns (HierarchyModel, exposures).  The model's rows are the file's, then
    the first `skybox_points` (pc_info.txt) rows of the scaffold in `scaffold_dir` with sigmoid
    opacities and their DC and three rest coefficients in a zero 16 x 3 block.  The anchors come from
    anchors.bin beside the file (absent: none, with a warning); exposures is the dict name -> (3, 4)
    tensor of exposure.json beside the file, or None when there is no such file (also kept as
    model.pretrained_exposures)."""
    from gaussian_hierarchy._C import load_hierarchy
    xyz, shs, alpha, log_scales, rots, nodes, boxes = load_hierarchy(hier_path)
    alpha = alpha.reshape(-1, 1)
    base = os.path.dirname(os.path.abspath(hier_path))
    anchors_path = os.path.join(base, ANCHORS_NAME)
    if os.path.exists(anchors_path):
        anchors = read_anchors(anchors_path)
    else:
        warnings.warn(f"load_hierarchy_model: no {ANCHORS_NAME} beside {hier_path}: no anchor rows are locked")
        anchors = torch.empty(0, dtype=torch.int64)
    exposures = None
    exposure_path = os.path.join(base, EXPOSURE_NAME)
    if os.path.exists(exposure_path):
        with open(exposure_path) as f:
            raw = json.load(f)
        exposures = {name: torch.tensor(v, dtype=torch.float32, device=device).reshape(3, 4) for name, v in raw.items()}
    skybox = 0
    if scaffold_dir:
        from .scaffold import load_scaffold
        sc = load_scaffold(scaffold_dir, device="cpu")
        skybox = sc.skybox_points
        if skybox > 0:
            s_xyz, s_ls, s_rot, s_op, s_shs = sc.skybox_rows()
            filler = torch.zeros(skybox, 16, 3)
            filler[:, :s_shs.shape[1]] = s_shs
            xyz, alpha = torch.cat((xyz, s_xyz)), torch.cat((alpha, s_op.reshape(-1, 1)))
            log_scales, rots = torch.cat((log_scales, s_ls)), torch.cat((rots, s_rot))
            shs = torch.cat((shs, filler))
    model = HierarchyModel(xyz, shs, alpha, torch.ones_like(log_scales), rots, nodes, boxes, skybox=skybox,
                           anchors=anchors, spatial_lr_scale=spatial_lr_scale, device=device)
    # HierarchyModel takes scales and stores their log; the file holds log-scales: stored as they are,
    # so a load -> save with no step in between reproduces the file
    model._scaling = torch.nn.Parameter(log_scales.to(device=device, dtype=torch.float32).contiguous())
    model.pretrained_exposures = exposures
    model.hierarchy_path = hier_path
    return model, exposures


@torch.no_grad()
def save_hier(model, path):
    """save_hier: every row (the appended skybox rows too, as the reference writes them), opacities
    through the model's abs activation, log-scales as stored.  `path` is written as given (the
    reference's caller appends "_opt")."""
    from gaussian_hierarchy._C import write_hierarchy
    write_hierarchy(path, model._xyz, model._features, torch.abs(model._opacity), model._scaling, model._rotation,
                    model.nodes, model.boxes)


def capture(step) -> dict:
    """The checkpoint of a post step: the five parameters, the optimizer's moments and step counts,
    the SH degree, the iteration and the host generator's state (the LOD limit is drawn from it) --
    tensors only, so torch.load(..., weights_only=True) reads it back."""
    m = step.m
    out = {"iteration": torch.tensor(step.iteration), "active_sh_degree": torch.tensor(m.active_sh_degree),
           "rng": torch.get_rng_state()}
    for n in _PARAMS:
        out["param" + n] = getattr(m, n).detach().clone()
    opt = step.optimizer
    for k, group in enumerate(opt.param_groups):
        st = opt.state.get(group["params"][0], {})
        for key in ("step", "exp_avg", "exp_avg_sq"):
            if key in st:
                out[f"opt{k}.{key}"] = st[key].clone()
    return out


@torch.no_grad()
def restore(step, state: dict) -> None:
    """Load a capture() into a step of either class built on the same hierarchy and views: the
    parameters and moments are replaced by new tensors (a native step then redoes its set-up)."""
    m = step.m
    dev = m._xyz.device
    opt = step.optimizer
    for k, group in enumerate(opt.param_groups):
        old = group["params"][0]
        name = next(n for n in _PARAMS if getattr(m, n) is old)
        newp = torch.nn.Parameter(state["param" + name].to(dev).clone().contiguous())
        setattr(m, name, newp)
        opt.state.pop(old, None)
        group["params"] = [newp]
        st = {key: state[f"opt{k}.{key}"].clone() for key in ("step", "exp_avg", "exp_avg_sq")
              if f"opt{k}.{key}" in state}
        for key in ("exp_avg", "exp_avg_sq"):
            if key in st:
                st[key] = st[key].to(dev).contiguous()
        if st:
            opt.state[newp] = st
    m.active_sh_degree = int(state["active_sh_degree"])
    step.iteration = int(state["iteration"])
    torch.set_rng_state(state["rng"])


class TrainPost:
    """Runs a step object through train_post.py's loop.  The views go in list order, repeated
    (:69-71: the loader is not shuffled); iteration `it` renders view (it - 1) % n.  The SH degree goes
    up at it % 1000 == 0 (:88-89): PostTrainStep and its subclasses do that in step(); for any other
    step object it is done here.  The last iteration that updates the model is iterations - 1: at
    `iterations` the reference renders, saves and returns before the optimizer (:159-165).

    on_save(it, model) fires at the save iterations with the model as the reference's scene.save sees
    it, that is before iteration it's update (:154-156 precede :191); on_checkpoint(it, capture dict)
    after it (:194-196)."""

    def __init__(self, step, iterations=15_000, save_iterations=(), checkpoint_iterations=(), on_save=None,
                 on_checkpoint=None):
        self.ts = step
        self.iterations = int(iterations)
        if getattr(step, "iterations", self.iterations) != self.iterations:
            raise ValueError("the step's schedules were built for a different iteration count")
        self.save_iterations = frozenset(int(i) for i in save_iterations)
        self.checkpoint_iterations = frozenset(int(i) for i in checkpoint_iterations)
        self.on_save = on_save
        self.on_checkpoint = on_checkpoint
        self._saved = set()

    def _save(self, it):
        if it in self.save_iterations and self.on_save is not None and it not in self._saved:
            self._saved.add(it)
            self.on_save(it, self.ts.m)

    def iteration(self):
        """One train_post.py iteration; returns the step's loss tensor."""
        ts = self.ts
        it = ts.iteration
        if not isinstance(ts, PostTrainStep):
            m = ts.m
            if it % 1000 == 0 and m.active_sh_degree < m.max_sh_degree:
                m.active_sh_degree += 1
        self._save(it)
        loss = ts.step()
        if it in self.checkpoint_iterations and self.on_checkpoint is not None:
            self.on_checkpoint(it, capture(ts))
        return loss

    def run(self, until=None, callback=None):
        """Iterations from the step's current one up to `until` (default: iterations - 1, the last one
        that updates the model; the save of iteration `iterations` then fires on the finished
        model).  callback(iteration, loss tensor) after each."""
        last = self.iterations - 1 if until is None else min(int(until), self.iterations - 1)
        while self.ts.iteration <= last:
            it = self.ts.iteration
            loss = self.iteration()
            if callback is not None:
                callback(it, loss)
        if self.ts.iteration == self.iterations:
            self._save(self.iterations)
