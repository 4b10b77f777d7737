"""CPU tests of the post-optimisation stage's files and loop (gs_train.post_stage): the .hier /
anchors.bin / exposure.json / scaffold round trips of load_hierarchy_model and save_hier on
device="cpu" models, and TrainPost's schedule with a stub step."""
from __future__ import annotations

import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hier_arrays(n, seed):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.randn(n, 3, generator=g)
    shs = torch.randn(n, 16, 3, generator=g)
    alpha = torch.rand(n, 1, generator=g) * 1.5  # activated; an interior node's may exceed 1
    log_scales = -4 + torch.randn(n, 3, generator=g)
    rots = torch.randn(n, 4, generator=g)
    nodes = torch.randint(0, 1000, (n, 7), generator=g, dtype=torch.int32)
    boxes = torch.randn(n, 2, 4, generator=g)
    return xyz, shs, alpha, log_scales, rots, nodes, boxes


def _write_hier(dir, n, seed):
    from gaussian_hierarchy._C import write_hierarchy
    a = _hier_arrays(n, seed)
    path = os.path.join(dir, "chunk.hier")
    write_hierarchy(path, a[0], a[1], a[2], a[3], a[4], a[5], a[6])
    return path, a


def _write_anchors(dir, rows, count_word=None):
    rows = np.asarray(rows, dtype="<i4")
    with open(os.path.join(dir, "anchors.bin"), "wb") as f:
        f.write(np.asarray([len(rows) if count_word is None else count_word], dtype="<u4").tobytes())
        f.write(rows.tobytes())


def _write_scaffold(dir, rows, skybox, seed):
    from gs_train.scaffold import save_scaffold
    g = torch.Generator().manual_seed(seed)
    m = types.SimpleNamespace(_xyz=torch.randn(rows, 3, generator=g), _opacity=torch.randn(rows, 1, generator=g),
                              _scaling=torch.randn(rows, 3, generator=g), _rotation=torch.randn(rows, 4, generator=g),
                              get_features=torch.randn(rows, 4, 3, generator=g))
    save_scaffold(dir, m, skybox)
    return m


@pytest.mark.parametrize("n", [3, 257])
@pytest.mark.parametrize("n_anchors", [0, 1, 1000])
@pytest.mark.parametrize("skybox", [None, 0, 7])
def test_load_save_round_trip(tmp_path, n, n_anchors, skybox):
    from gs_train.post_stage import load_hierarchy_model, save_hier
    d = str(tmp_path)
    path, a = _write_hier(d, n, seed=n + n_anchors)
    anchors = np.random.default_rng(n_anchors).integers(0, n, n_anchors)
    # the count word disagrees with the payload: ignored, as the reference ignores it
    _write_anchors(d, anchors, count_word=n_anchors + 5)
    expo = {"img_%d.jpg" % k: (np.eye(3, 4) + 0.01 * k).tolist() for k in range(3)}
    with open(os.path.join(d, "exposure.json"), "w") as f:
        json.dump(expo, f)
    sdir = None
    if skybox is not None:
        sdir = os.path.join(d, "scaffold")
        sc = _write_scaffold(sdir, 20, skybox, seed=5)
    model, exposures = load_hierarchy_model(path, scaffold_dir=sdir, spatial_lr_scale=2.5, device="cpu")
    S = skybox or 0
    assert model.N == n + S and model.skybox_points == S and model.spatial_lr_scale == 2.5
    assert model.anchors.dtype == torch.int64 and model.anchors.tolist() == anchors.tolist()
    assert set(exposures) == set(expo)
    for k, v in expo.items():
        assert exposures[k].shape == (3, 4)
        assert torch.equal(exposures[k], torch.tensor(v, dtype=torch.float32))
    # the node rows are the file's, bit for bit (the log-scales are stored, not exp'd and log'd)
    for got, want in zip((model._xyz, model._features, model._opacity, model._scaling, model._rotation),
                         (a[0], a[1], a[2], a[3], a[4])):
        assert torch.equal(got.detach()[:n], want)
    assert torch.equal(model.nodes, a[5]) and torch.equal(model.boxes, a[6])
    if S:
        # the skybox rows in order, after the node rows: sigmoid opacities, DC + three rest
        # coefficients in a zero 16 x 3 block
        assert torch.equal(model._xyz.detach()[n:], sc._xyz[:S])
        assert torch.equal(model._scaling.detach()[n:], sc._scaling[:S])
        assert torch.equal(model._rotation.detach()[n:], sc._rotation[:S])
        assert torch.equal(model._opacity.detach()[n:], torch.sigmoid(sc._opacity[:S]))
        assert torch.equal(model._features.detach()[n:, :4], sc.get_features[:S])
        assert torch.count_nonzero(model._features.detach()[n:, 4:]) == 0
    out = os.path.join(d, "chunk.hier_opt")
    save_hier(model, out)
    src, dst = open(path, "rb").read(), open(out, "rb").read()
    if S == 0:
        assert src == dst  # load -> save with no step: every byte
    else:
        from gaussian_hierarchy._C import load_hierarchy
        back = load_hierarchy(out)
        assert back[0].shape[0] == n + S  # every row is written, the skybox rows too
        for got, want in zip(back[:5], a[:5]):
            assert torch.equal(got[:n].reshape(want.shape), want)
        assert torch.equal(back[5], a[5]) and torch.equal(back[6], a[6])
        assert torch.equal(back[2][n:].reshape(-1, 1), torch.sigmoid(sc._opacity[:S]))


def test_save_hier_writes_abs_opacity_and_log_scales(tmp_path):
    from gaussian_hierarchy._C import load_hierarchy
    from gs_train.post_stage import load_hierarchy_model, save_hier
    path, a = _write_hier(str(tmp_path), 3, seed=1)
    _write_anchors(str(tmp_path), [])
    model, _ = load_hierarchy_model(path, device="cpu")
    with torch.no_grad():
        model._opacity[1] = -0.25  # an optimizer step may take a stored opacity below zero
    out = str(tmp_path / "o.hier")
    save_hier(model, out)
    back = load_hierarchy(out)
    assert torch.equal(back[2].reshape(-1), model._opacity.detach().abs().reshape(-1))
    assert torch.equal(back[3], a[3])


def test_missing_anchors_and_exposure(tmp_path):
    from gs_train.post_stage import load_hierarchy_model
    path, _ = _write_hier(str(tmp_path), 3, seed=2)
    with pytest.warns(UserWarning, match="anchors.bin"):
        model, exposures = load_hierarchy_model(path, device="cpu")
    assert model.anchors.numel() == 0 and model.anchors.dtype == torch.int64
    assert exposures is None and model.pretrained_exposures is None


def test_truncated_anchors_payload_raises(tmp_path):
    from gs_train.post_stage import load_hierarchy_model
    path, _ = _write_hier(str(tmp_path), 3, seed=3)
    with open(os.path.join(str(tmp_path), "anchors.bin"), "wb") as f:
        f.write(np.asarray([2], dtype="<u4").tobytes() + np.asarray([0, 1], dtype="<i4").tobytes()[:-1])
    with pytest.raises(ValueError, match="anchors.bin"):
        load_hierarchy_model(path, device="cpu")


class _StubStep:
    """Records what TrainPost asks of a step (not a PostTrainStep: TrainPost raises its SH degree)."""

    def __init__(self, n_views, iterations, degree=0):
        self.m = types.SimpleNamespace(active_sh_degree=degree, max_sh_degree=3,
                                       **{n: torch.zeros(2, 1) for n in ("_xyz", "_features", "_opacity", "_scaling",
                                                                         "_rotation")})
        self.optimizer = types.SimpleNamespace(param_groups=[], state={})
        self.iterations = iterations
        self.iteration = 1
        self.n_views = n_views
        self.views, self.degrees = [], []

    def step(self):
        self.views.append((self.iteration - 1) % self.n_views)
        self.degrees.append(self.m.active_sh_degree)
        self.iteration += 1
        return torch.tensor(float(self.iteration))


def test_train_post_schedule():
    from gs_train.post_stage import TrainPost
    st = _StubStep(3, 2500)
    saves, ckpts, seen = [], [], []
    tp = TrainPost(st, iterations=2500, save_iterations=(7, 2500), checkpoint_iterations=(5, 2499, 2500),
                   on_save=lambda it, m: saves.append((it, st.iteration, m is st.m)),
                   on_checkpoint=lambda it, c: ckpts.append((it, int(c["iteration"]))))
    tp.run(until=10, callback=lambda it, loss: seen.append(it))
    assert seen == list(range(1, 11)) and st.iteration == 11
    assert st.views == [(i - 1) % 3 for i in range(1, 11)]  # list order, repeated
    assert saves == [(7, 7, True)]          # before iteration 7's update
    assert ckpts == [(5, 6)]                # after iteration 5's
    tp.run()
    # the last iteration that updates the model is iterations - 1; the save of `iterations` sees the
    # finished model, and no checkpoint is taken there (the reference returns first)
    assert st.iteration == 2500 and len(st.views) == 2499
    assert saves == [(7, 7, True), (2500, 2500, True)]
    assert ckpts == [(5, 6), (2499, 2500)]
    # oneupSHdegree at it % 1000 == 0
    assert st.degrees[998] == 0 and st.degrees[999] == 1 and st.degrees[1999] == 2 and st.m.active_sh_degree == 2
    tp.run()  # nothing left: no further iteration, no second save
    assert len(st.views) == 2499 and len(saves) == 2


def test_train_post_rejects_other_iteration_count():
    from gs_train.post_stage import TrainPost
    with pytest.raises(ValueError):
        TrainPost(_StubStep(2, 100), iterations=200)


def test_post_header_symbols_are_exported_and_typed():
    """include/gsr_post.h against the library and _lib.POST_SIGNATURES (the table load() types)."""
    from diff_gaussian_rasterization import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gsr_post.h")).read(), flags=re.S)
    syms = set(re.findall(r"\b(gsr_[a-z_0-9]+)\s*\(", text))
    assert len(syms) == 8 and syms == set(_lib.POST_SIGNATURES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s
    assert _lib.load().gsr_abi_version() == 7
    # the ctypes mirror of gsr_post_step_args: the C layout's size (LP64: 8-byte pointers and int64)
    assert ctypes.sizeof(_lib.PostStepArgs) == 304
