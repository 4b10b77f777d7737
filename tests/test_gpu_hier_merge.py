"""GPU tests of the hierarchy merger (csrc/hier_merge.hip through gs_train.hier_merge) against its
numpy restatement tests/hier_merge_ref.py (the rule: DESIGN.md "Hierarchy merger"; parity unpinned
against the un-vendored gaussianhierarchy tool).

The chunk hierarchies come from build_hierarchy on the device; their attributes are then moved as
train_post would move them, some opacities set negative by hand, and some leaves' means edited by the
case (hier_merge_ref.finish_case).

Exact: nodes, source, leaf_rows, levels and the per-chunk K_c equal the reference's; retained rows and
boxes are bit copies of the chunks' rows; a new top box is the bitwise union of the device's own
children's boxes; boxes[:, 0, 3] is the fp32 largest extent; two merges are bitwise equal; .save then
load_hierarchy round-trips; the device's cut of the merged arrays covers every surviving leaf exactly once.

Toleranced, new top nodes only, and local as in DESIGN 14.3: the device's own two child rows go through
the float64 step E (with |opacity|), and the device's merged row is compared with that.  The bounds are
4 x the largest error a float32 numpy evaluation of the same step shows against float64 on these
cases' own top-tree steps (hier_merge_ref.fp32_basis(), run on a CPU; `python tests/hier_merge_ref.py`
prints them) -- the margin covers another operation order, the device's powf and its Jacobi iteration
against eigh.  Nothing here is derived from the device's output.

The sizes: P = 64 / 65 straddle a wave; C = 70 gives a top tree of several levels whose 139 nodes
straddle a wave; C = 257 is one more than the ownership kernel's centre batch; C = 4 x P = 20 000
(159 996 input nodes) crosses the 256-node workgroups of every per-node launch and the 1024-node tiles of
the numbering, with levels of many tiles."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hier_build_ref as R  # noqa: E402
import hier_merge_ref as MR  # noqa: E402

DEV = "cuda"

# hier_merge_ref.fp32_basis() over MR.CASES, measured on a CPU (numpy float32 against float64) on the
# top-tree steps: mu and SH relative to the larger child norm, opacity (W / S) relative, R diag(s^2) R^T
# against the mixture covariance in relative Frobenius norm.
FP32_MEASURED = dict(mu=1.401e-07, sh=1.532e-07, opacity=5.923e-07, cov=5.295e-07)
BOUNDS = {k: 4.0 * v for k, v in FP32_MEASURED.items()}
UNIT_QUAT_TOL = 4 * 2.0 ** -23

_cache = {}
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def _t(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _built(cl):
    from gs_train.hier_build import build_hierarchy
    h = build_hierarchy(_t(cl["xyz"]), _t(cl["log_scales"]), _t(cl["rotations"]), _t(cl["opacities"]), _t(cl["shs"]))
    return dict(nodes=h.nodes.cpu().numpy(), boxes=h.boxes.cpu().numpy(), means3D=h.means3D.cpu().numpy(),
                log_scales=h.log_scales.cpu().numpy(), rotations=h.rotations.cpu().numpy(),
                opacities=h.opacities.cpu().numpy(), shs=h.shs.cpu().numpy())


def _hier(ch):
    from gs_train.hier_build import Hierarchy
    nodes = _t(ch["nodes"], torch.int32)
    leaf_rows = torch.where(nodes[:, 6] == 0, nodes[:, 2], torch.full_like(nodes[:, 2], -1))
    return Hierarchy(_t(ch["means3D"]), _t(ch["log_scales"]), _t(ch["rotations"]), _t(ch["opacities"]), _t(ch["shs"]),
                     nodes, _t(ch["boxes"]), leaf_rows, int(ch["nodes"][:, 0].max()) + 1)


def _np(m):
    return dict(means3D=m.means3D.cpu().numpy(), log_scales=m.log_scales.cpu().numpy(), rotations=m.rotations.cpu().numpy(),
                opacities=m.opacities.cpu().numpy(), shs=m.shs.cpu().numpy(), nodes=m.nodes.cpu().numpy(),
                boxes=m.boxes.cpu().numpy(), leaf_rows=m.leaf_rows.cpu().numpy(), source=m.source.cpu().numpy(),
                levels=m.levels, K_c=list(m.chunk_leaves))


def _chunks(name):
    """The case's chunks (numpy, built on the device and then perturbed) and centres: made once."""
    if ("chunks", name) not in _cache:
        clouds, centres = MR.case_clouds(name)
        _cache["chunks", name] = (MR.finish_case(name, [_built(cl) for cl in clouds]), centres)
    return _cache["chunks", name]


def _case(name):
    """The chunks, the centres, the reference's merge and the device's: made once, never modified."""
    from gs_train.hier_merge import merge_hierarchies
    if name not in _cache:
        chunks, centres = _chunks(name)
        hs = [_hier(c) for c in chunks]
        m = merge_hierarchies(hs, torch.from_numpy(centres))
        _cache[name] = (chunks, centres, MR.merge(chunks, centres), _np(m), m, hs)
    return _cache[name]


CASES = pytest.mark.parametrize("name", MR.CASES)


@pytest.mark.gpu
@CASES
def test_layout_source_and_counts_equal_the_reference(name):
    chunks, centres, ref, d, _, _ = _case(name)
    K = sum(ref["K_c"])
    assert d["K_c"] == ref["K_c"]
    assert d["nodes"].shape == (2 * K - 1, 7) and d["nodes"].dtype == np.int32 and d["source"].dtype == np.int32
    assert d["levels"] == ref["levels"]
    assert np.array_equal(d["source"], ref["source"])
    assert np.array_equal(d["nodes"], ref["nodes"])
    assert np.array_equal(d["leaf_rows"], ref["leaf_rows"])


@pytest.mark.gpu
@CASES
def test_retained_rows_are_bit_copies_and_top_boxes_exact_unions(name):
    chunks, centres, ref, d, _, _ = _case(name)
    src, b = d["source"], d["boxes"]
    M = d["shs"].shape[1]
    assert M == max(c["shs"].shape[1] for c in chunks)
    for c, ch in enumerate(chunks):
        sel = np.nonzero(src[:, 0] == c)[0]
        old = src[sel, 1]
        for k in ("means3D", "log_scales", "rotations", "opacities"):
            assert np.array_equal(bits(d[k][sel]), bits(ch[k][old])), (c, k)  # the opacity sign too
        Mc = ch["shs"].shape[1]
        assert np.array_equal(bits(d["shs"][sel, :Mc]), bits(ch["shs"][old])) and not d["shs"][sel, Mc:].any()
        assert np.array_equal(bits(b[sel]), bits(ch["boxes"][old])), c
    top = np.nonzero(src[:, 0] < 0)[0]
    ca = d["nodes"][top, 5]
    assert np.array_equal(bits(b[top, 0, :3]), bits(np.minimum(b[ca, 0, :3], b[ca + 1, 0, :3])))
    assert np.array_equal(bits(b[top, 1, :3]), bits(np.maximum(b[ca, 1, :3], b[ca + 1, 1, :3])))
    assert np.array_equal(bits(b), bits(ref["boxes"]))
    assert np.array_equal(bits(b[:, 0, 3]), bits(R.box_extent(b)))
    assert not b[:, 1, 3].any()


@pytest.mark.gpu
@CASES
def test_top_rows_against_the_float64_step_on_the_devices_own_children(name):
    chunks, centres, ref, d, _, _ = _case(name)
    idx, a, b, got = MR.top_children(d)
    assert len(idx) == sum(k > 0 for k in ref["K_c"]) - 1
    if not len(idx):
        return
    e = R.step_errors(got, R.merge_step(a, b), a, b)
    print(name, {k: f"{v:.3e}" for k, v in e.items()})
    for k, v in e.items():
        assert v <= BOUNDS[k], (k, v, BOUNDS[k])
    q = got["rotations"].astype(np.float64)
    assert (np.abs((q * q).sum(1) - 1.0) <= UNIT_QUAT_TOL).all()
    assert np.isfinite(got["log_scales"]).all() and np.isfinite(got["xyz"]).all() and (got["opacities"] >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c3_mixed", "c70_p300"])
def test_two_merges_are_bitwise_equal(name):
    from gs_train.hier_merge import merge_hierarchies
    chunks, centres, ref, d, _, hs = _case(name)
    again = _np(merge_hierarchies(hs, torch.from_numpy(centres)))
    for k, v in d.items():
        if k in ("levels", "K_c"):
            assert again[k] == v
        else:
            assert np.array_equal(np.ascontiguousarray(again[k]).view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), k


@pytest.mark.gpu
def test_one_chunk_that_owns_everything_comes_back_bit_for_bit():
    chunks, centres, ref, d, _, _ = _case("c1_p1000")
    ch = chunks[0]
    assert np.array_equal(d["nodes"], ch["nodes"])
    for k in ("means3D", "log_scales", "rotations", "opacities", "shs", "boxes"):
        assert np.array_equal(bits(d[k]), bits(ch[k])), k
    assert np.array_equal(d["source"][:, 1], np.arange(1999)) and not d["source"][:, 0].any()
    chunks, centres, ref, d, _, _ = _case("c1_p1")
    assert d["nodes"].tolist() == [[0, -1, 0, 1, 0, -1, 0]] and d["levels"] == 1 and d["K_c"] == [1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2_p64_p65", "c3_mixed"])
def test_save_and_load_round_trip(name, tmp_path):
    from gaussian_hierarchy._C import load_hierarchy
    _, _, _, d, m, _ = _case(name)
    path = str(tmp_path / "merged.hier")
    m.save(path)
    xyz, shs, alpha, scales, rots, nodes, boxes = load_hierarchy(path)
    for got, k in ((xyz, "means3D"), (alpha, "opacities"), (scales, "log_scales"), (rots, "rotations"), (boxes, "boxes")):
        assert np.array_equal(bits(got.numpy()), bits(d[k])), k
    M = d["shs"].shape[1]
    assert np.array_equal(bits(shs[:, :M].numpy()), bits(d["shs"])) and not shs[:, M:].any()
    assert np.array_equal(nodes.numpy(), d["nodes"])
    model = m.to_model()
    assert model.N == d["nodes"].shape[0] and torch.equal(model._xyz, m.means3D)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2_p64_p65", "nan_leaves", "c70_p300"])
def test_device_cut_of_the_merged_arrays_covers_every_surviving_leaf_once(name):
    from gaussian_hierarchy._C import expand_to_size
    _, _, _, d, m, _ = _case(name)
    N = d["nodes"].shape[0]
    ri, pi, ni = (torch.zeros(N, dtype=torch.int32, device=DEV) for _ in range(3))
    lengths = []
    for v in MR.VIEWPOINTS:
        for target in MR.targets(d["boxes"], v):
            n = expand_to_size(m.nodes, m.boxes, float(target), torch.tensor(v, device=DEV), torch.zeros(3), ri, pi, ni)
            MR.assert_cut_covers_each_leaf_once(d["nodes"], ni[:n].cpu().numpy())
            assert torch.equal(ri[:n], ni[:n])
            lengths.append(n)
        assert sorted(ni[:n].tolist()) == np.nonzero(d["nodes"][:, 6] == 0)[0].tolist()  # target 0: the leaves
    assert lengths[0] < lengths[2]


@pytest.mark.gpu
def test_command_line_merges_hier_opt_files_with_skybox_rows(tmp_path):
    from gaussian_hierarchy._C import load_hierarchy, write_hierarchy
    from gs_train import hier_merge as HM
    chunks, centres, ref, d, _, hs = _case("c2_p64_p65")
    names = ["0_0", "1_0"]
    g = torch.Generator().manual_seed(3)
    for name, h, cen in zip(names, hs, centres):
        os.makedirs(tmp_path / "chunks" / name)
        os.makedirs(tmp_path / "trained" / name)
        (tmp_path / "chunks" / name / "center.txt").write_text(" ".join(repr(float(v)) for v in cen) + "\n")
        S = 7  # save_hier writes the skybox rows after the node rows
        sky = lambda t: torch.cat([t.cpu(), torch.rand((S,) + tuple(t.shape[1:]), generator=g)])
        write_hierarchy(str(tmp_path / "trained" / name / "hierarchy.hier_opt"), sky(h.means3D), sky(h._shs16()),
                        sky(h.opacities), sky(h.log_scales), sky(h.rotations), h.nodes, h.boxes)
    out = str(tmp_path / "merged.hier")
    assert HM.main([str(tmp_path / "trained"), "0", str(tmp_path / "chunks"), out] + names, device=DEV) == 0
    xyz, shs, alpha, scales, rots, nodes, boxes = load_hierarchy(out)
    assert np.array_equal(nodes.numpy(), d["nodes"]) and np.array_equal(bits(boxes.numpy()), bits(d["boxes"]))
    for got, k in ((xyz, "means3D"), (alpha, "opacities"), (scales, "log_scales"), (rots, "rotations"), (shs, "shs")):
        assert np.array_equal(bits(got.numpy()), bits(d[k])), k


@pytest.mark.gpu
def test_no_surviving_leaf_raises():
    from gs_train.hier_merge import merge_hierarchies
    chunks, centres = _chunks("all_nonfinite")
    with pytest.raises(RuntimeError, match="no chunk has a surviving leaf"):
        merge_hierarchies([_hier(c) for c in chunks], torch.from_numpy(centres))


@pytest.mark.gpu
@pytest.mark.parametrize("col,value,what", [(1, None, "parent >= id"), (4, 2, "count_merged = 2")])
def test_a_chunk_that_breaks_the_layout_is_refused(col, value, what):
    from gs_train.hier_merge import merge_hierarchies
    chunks, centres = _chunks("c2_p64_p65")
    nodes = chunks[1]["nodes"].copy()
    n = int(np.nonzero(nodes[:, 6] == 2)[0][5])
    nodes[n, col] = n + 3 if value is None else value
    bad = MR.validate(nodes)  # the first offending node: n, or n's parent, whose child no longer names it
    assert 0 <= bad <= n
    hs = [_hier(chunks[0]), _hier(dict(chunks[1], nodes=nodes))]
    with pytest.raises(RuntimeError, match=f"chunk 1: node {bad} breaks the hierarchy layout"):
        merge_hierarchies(hs, torch.from_numpy(centres))


@pytest.mark.gpu
def test_stage_times_and_scratch():
    from gs_train import hier_merge as HM
    chunks, centres, ref, d, _, hs = _case("c2_slab")
    HM.merge_hierarchies(hs, torch.from_numpy(centres))
    ms = HM.stage_ms()
    assert tuple(ms) == HM.STAGES and all(v >= 0 for v in ms.values()) and ms["gather"] > 0 and ms["ownership"] > 0
    T = sum(c["nodes"].shape[0] for c in chunks)
    assert 0 < HM.scratch_bytes(2, T) < 32 * T + (1 << 20)
    # the slab: chunk 0 keeps a small part of its cloud, so chains of spliced nodes are long
    kept = ref["K_c"][0]
    assert 0 < kept < 150
