"""CPU checks of the LOD hierarchy builder's rule (DESIGN.md "Hierarchy builder") as restated in
tests/hier_build_ref.py, the checker of csrc/hier_build.hip, and of the builder's host surface: the
ctypes table against include/gsr_hier_build.h and the library, the argument errors of the C entry
points and of gs_train.hier_build.build_hierarchy without a GPU, and a .save() -> load_hierarchy round
trip.

The gaussianhierarchy tool is not vendored in the reference, so parity against it is UNPINNED.  What is
pinned here, on the restatement: every input row is a leaf exactly once, the breadth-first layout, box
containment, the weights' additivity, the root's moments against the leaves' mixture (fp64, 1e-9), and
that the unchanged cut oracle (gso_expand_to_size) returns proper cuts of the tree."""
from __future__ import annotations

import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hier_build_ref as R  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gsr_hier_build.h")
ENTRY_POINTS = {"gsr_hier_build_scratch_bytes", "gsr_hier_build", "gsr_hier_build_stage_ms"}

PROBLEMS = [("random", 1), ("random", 2), ("random", 3), ("random", 3000), ("ties", 600), ("planar", 500),
            ("identical", 300)]
_built = {}


def _problem(kind, P):
    if (kind, P) not in _built:
        c = R.cloud(kind, P, M=4, seed=P)
        _built[kind, P] = (c, R.build(**c))
    return _built[kind, P]


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(gsr_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out


def test_lib_declares_the_header_entry_points():
    from diff_gaussian_rasterization import _lib
    decl = _declarations()
    assert set(decl) == ENTRY_POINTS
    table = _lib.HIER_BUILD_SIGNATURES
    assert set(table) == set(decl), "ctypes table out of sync with include/gsr_hier_build.h"
    for name, n in decl.items():
        assert len(table[name][1]) == n, f"{name}: {len(table[name][1])} ctypes arguments, the header has {n}"
    assert not set(table) & (set(_lib.SIGNATURES) | set(_lib.GT_SIGNATURES) | set(_lib.EVAL_SIGNATURES))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), f"libgsr_hip.so does not export {name}"
    L = _lib.load()
    assert L.gsr_hier_build_scratch_bytes.restype is ctypes.c_size_t
    assert L.gsr_abi_version() == 7


def test_native_calls_validate_without_gpu():
    """Argument checks return before any device work."""
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    assert L.gsr_hier_build_scratch_bytes(0) == 0 and L.gsr_hier_build_scratch_bytes((1 << 30) + 1) == 0
    need = L.gsr_hier_build_scratch_bytes(1000)
    assert 0 < need < 1000 * 64 + (1 << 20)
    assert L.gsr_hier_build_scratch_bytes(2000) >= need
    one = ctypes.c_void_p(16)  # never dereferenced: the calls fail on their arguments
    lv = ctypes.c_int(7)
    ptrs = [one] * 13

    def call(P, M, p=ptrs, levels=ctypes.byref(lv), scratch=one, nbytes=1 << 40):
        return L.gsr_hier_build(P, M, *p, levels, scratch, nbytes, None)

    for P in (0, -5, (1 << 30) + 1):
        assert call(P, 16) == -1 and b"gsr_hier_build" in L.gsr_last_error()
    for M in (0, 17, -1):
        assert call(10, M) == -1 and b"M must be" in L.gsr_last_error()
    for k in range(13):
        assert call(10, 16, p=ptrs[:k] + [None] + ptrs[k + 1:]) == -1 and b"NULL" in L.gsr_last_error()
    assert call(10, 16, levels=None) == -1 and call(10, 16, scratch=None) == -1
    assert call(1000, 16, nbytes=need - 1) == -1 and b"scratch too small" in L.gsr_last_error()
    assert call(10, 16, p=ptrs[:2] + [ctypes.c_void_p(20)] + ptrs[3:]) == -1 and b"aligned" in L.gsr_last_error()
    assert lv.value == 0  # reset by every call
    buf = (ctypes.c_float * 4)()
    assert L.gsr_hier_build_stage_ms(buf, 4) == 4 and L.gsr_hier_build_stage_ms(None, 4) == 0


def test_build_hierarchy_argument_errors_without_gpu():
    from gs_train.hier_build import build_hierarchy
    c = {k: torch.from_numpy(v) for k, v in R.cloud("random", 8, M=4).items()}
    args = lambda **kw: [dict(c, **kw)[k] for k in ("xyz", "log_scales", "rotations", "opacities", "shs")]
    with pytest.raises(ValueError):
        build_hierarchy(*args(xyz=c["xyz"][:7]))
    with pytest.raises(ValueError):
        build_hierarchy(*args(log_scales=c["log_scales"][:, :2]))
    with pytest.raises(ValueError):
        build_hierarchy(*args(rotations=c["rotations"][:, :3]))
    with pytest.raises(ValueError):
        build_hierarchy(*args(opacities=c["opacities"][:5]))
    with pytest.raises(ValueError):
        build_hierarchy(*args(shs=torch.zeros(8, 17, 3)))
    with pytest.raises(ValueError):
        build_hierarchy(*args(shs=torch.zeros(8, 0, 3)))
    with pytest.raises(ValueError):
        build_hierarchy(*args(xyz=c["xyz"].double()))
    with pytest.raises(ValueError):
        build_hierarchy(*args(), first_row=8)
    with pytest.raises(TypeError):
        build_hierarchy(*args(xyz=c["xyz"].numpy()))
    # valid arguments on the CPU: refused as not on a GPU (there is no CPU path)
    with pytest.raises(RuntimeError):
        build_hierarchy(*args())


def test_keys_interleave_as_synthetic_morton3_and_quantise_by_one_cube():
    from gs_train.synthetic import _morton3
    rng = np.random.default_rng(0)
    q = rng.integers(0, 2 ** 20, (1000, 3))
    mine = (R._spread21(q[:, 0].astype(np.uint64)) | (R._spread21(q[:, 1].astype(np.uint64)) << np.uint64(1))
            | (R._spread21(q[:, 2].astype(np.uint64)) << np.uint64(2)))
    assert np.array_equal(mine.astype(np.int64), _morton3(q.astype(np.int64)))
    assert int(R._spread21(np.uint64(2 ** 21 - 1))) == 0x1249249249249249  # 21 bits, every third
    # one cube scale: x spans 8, y spans 2 -> y's cells end at a quarter of the range; the far corner clamps
    xyz = np.array([[0, 0, 0], [8, 2, 0], [4, 1, 0]], np.float32)
    k = R.morton_keys(xyz)
    assert int(k[0]) == 0
    assert int(k[1]) == int(R._spread21(np.uint64(2 ** 21 - 1))) | int(R._spread21(np.uint64(2 ** 19))) << 1
    assert int(k[2]) == int(R._spread21(np.uint64(2 ** 20))) | int(R._spread21(np.uint64(2 ** 18))) << 1
    assert not R.morton_keys(np.ones((5, 3), np.float32)).any()  # ext = 0


def test_split_bisection_equals_the_definition():
    for kind, P in (("ties", 200), ("random", 150), ("identical", 40)):
        keys = R.morton_keys(R.cloud(kind, P, M=1, seed=5)["xyz"])
        a = R.topology(keys)
        b = R.topology(keys, split_fn=R.split_by_scan)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_tie_break_splits_equal_keys_by_position():
    keys = np.zeros(5, np.uint64)  # delta = 64 + clz32(a ^ b): [0..4] -> [0..3] | [4], [0..1] | [2..3]
    nodes, leaf_rows, levels = R.topology(keys)
    assert levels == 4 and nodes[0, 5] == 1
    assert leaf_rows.tolist() == [-1, -1, 4, -1, -1, 0, 1, 2, 3]


@pytest.mark.parametrize("kind,P", PROBLEMS)
def test_layout_properties(kind, P):
    c, h = _problem(kind, P)
    nodes, leaf_rows = h["nodes"], h["leaf_rows"]
    N = 2 * P - 1
    assert nodes.shape == (N, 7) and nodes.dtype == np.int32 and h["levels"] == nodes[:, 0].max() + 1
    assert h["levels"] <= 96
    # every input row is a leaf exactly once
    leaf = leaf_rows >= 0
    assert sorted(leaf_rows[leaf].tolist()) == list(range(P))
    assert np.array_equal(nodes[0, :2], (0, -1)) and np.array_equal(nodes[:, 2], np.arange(N))
    assert np.array_equal(nodes[leaf, 3:], np.tile((1, 0, -1, 0), (P, 1)))
    inner = np.nonzero(~leaf)[0]
    assert np.array_equal(nodes[inner, 3:5], np.tile((0, 1), (P - 1, 1))) and (nodes[inner, 6] == 2).all()
    # breadth-first: depths do not decrease, consecutive interior nodes' children are consecutive
    assert (np.diff(nodes[:, 0]) >= 0).all()
    assert np.array_equal(nodes[inner, 5], 1 + 2 * np.arange(P - 1))
    for n in inner:
        ca = nodes[n, 5]
        assert (nodes[ca:ca + 2, 1] == n).all() and (nodes[ca:ca + 2, 0] == nodes[n, 0] + 1).all()
    # leaves are bit copies (the reference holds them as float64 of the fp32 inputs)
    assert np.array_equal(h["means3D"][leaf].astype(np.float32), c["xyz"][leaf_rows[leaf]])
    assert np.array_equal(h["rotations"][leaf].astype(np.float32), c["rotations"][leaf_rows[leaf]])
    # every parent box contains its children; size = the largest extent
    b = h["boxes"].astype(np.float32)  # as the cut reads them; the reference's leaf boxes are float64
    ca = nodes[inner, 5]
    for k in (ca, ca + 1):
        assert (b[k, 0, :3] >= b[inner, 0, :3]).all() and (b[k, 1, :3] <= b[inner, 1, :3]).all()
    assert (b[:, 1, :3] >= b[:, 0, :3]).all() and (b[:, 1, 3] == 0).all()
    assert np.array_equal(b[:, 0, 3].astype(np.float32), R.box_extent(b.astype(np.float32)))
    q = h["rotations"][inner]
    assert np.allclose((q * q).sum(1), 1.0, atol=1e-12) and np.isfinite(h["log_scales"]).all()


@pytest.mark.parametrize("kind,P", PROBLEMS)
def test_weights_add_up_and_root_moments_are_the_leaves_mixture(kind, P):
    c, h = _problem(kind, P)
    nodes, leaf_rows, W = h["nodes"], h["leaf_rows"], h["W"]
    N = nodes.shape[0]
    leaf = leaf_rows >= 0
    cov_l, s_l = R.row_cov(c["log_scales"].astype(np.float64), c["rotations"].astype(np.float64))
    w = c["opacities"].reshape(-1).astype(np.float64) * R.surface(s_l)
    # each node's W is the sum of its leaves' w
    sums = np.zeros(N)
    sums[leaf] = w[leaf_rows[leaf]]
    for n in range(N - 1, 0, -1):  # children are stored after their parents
        sums[nodes[n, 1]] += sums[n]
    assert np.allclose(W, sums, rtol=1e-9, atol=0)
    # a node's stored opacity x surface gives W back (what its parent's merge reads)
    assert np.allclose(h["opacities"] * R.surface(np.exp(h["log_scales"])), W, rtol=1e-9, atol=0)
    x = c["xyz"].astype(np.float64)
    mu = (w[:, None] * x).sum(0) / w.sum()
    d = x - mu
    cov = (w[:, None, None] * (cov_l + d[:, :, None] * d[:, None, :])).sum(0) / w.sum()
    assert np.linalg.norm(h["means3D"][0] - mu) <= 1e-9 * np.linalg.norm(mu)
    root = R.cov_of_rows(h["log_scales"][:1], h["rotations"][:1])[0]
    assert np.linalg.norm(root - cov) <= 1e-9 * np.linalg.norm(cov)
    sh = (w[:, None] * c["shs"].reshape(P, -1)).sum(0) / w.sum()
    assert np.linalg.norm(h["shs"][0].reshape(-1) - sh) <= 1e-9 * np.linalg.norm(sh)


def _assert_proper_cut(nodes, ni):
    """Every leaf has exactly one ancestor-or-self among the rendered nodes ni."""
    N = nodes.shape[0]
    assert len(np.unique(ni)) == len(ni)
    cover = np.zeros(N, np.int64)
    cover[ni] = 1
    for n in range(1, N):  # parents are stored before their children
        cover[n] += cover[nodes[n, 1]]
    assert (cover[nodes[:, 6] == 0] == 1).all()


@pytest.mark.parametrize("kind,P", PROBLEMS)
def test_unchanged_cut_oracle_returns_proper_cuts(kind, P):
    import gs_oracle as O
    c, h = _problem(kind, P)
    nodes, boxes = h["nodes"], h["boxes"].astype(np.float32)
    v = np.array([0.0, 0.0, -50.0], np.float32)  # outside every box
    ri, pi, ni = O.expand_to_size(nodes, boxes, np.float32(1e30), v)
    assert ni.tolist() == [0] and pi.tolist() == [-1]  # a huge target: the root alone
    ri, pi, ni = O.expand_to_size(nodes, boxes, np.float32(0.0), v)
    assert sorted(ni.tolist()) == np.nonzero(nodes[:, 6] == 0)[0].tolist() and len(ni) == P  # target 0: the leaves
    _assert_proper_cut(nodes, ni)
    root = float(boxes[0, 0, 3]) / 52.0  # about the root's projected size
    lengths = []
    for frac in (0.3, 0.1, 0.03):
        ri, pi, ni = O.expand_to_size(nodes, boxes, np.float32(root * frac), v)
        _assert_proper_cut(nodes, ni)
        assert np.array_equal(ri, ni)  # Gaussian row n belongs to node n
        lengths.append(len(ni))
    if kind == "random" and P == 3000:
        assert 1 < lengths[0] < lengths[1] < lengths[2] < P


def test_save_and_load_round_trip(tmp_path):
    from gaussian_hierarchy._C import load_hierarchy
    from gs_train.hier_build import Hierarchy
    c, h = _problem("random", 3000)  # M = 4: the file holds 16 coefficients, the rest zero
    N = h["nodes"].shape[0]
    t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a)).to(dt)
    hier = Hierarchy(t(h["means3D"]), t(h["log_scales"]), t(h["rotations"]), t(h["opacities"]).reshape(N, 1),
                     t(h["shs"]), t(h["nodes"], torch.int32), t(h["boxes"]), t(h["leaf_rows"], torch.int32), h["levels"])
    path = str(tmp_path / "chunk.hier")
    hier.save(path)
    assert os.path.getsize(path) == 4 + N * (3 + 4 + 3 + 1 + 48) * 4 + 4 + N * 7 * 4 + N * 8 * 4
    xyz, shs, alpha, scales, rots, nodes, boxes = load_hierarchy(path)
    assert torch.equal(xyz, hier.means3D) and torch.equal(alpha, hier.opacities) and torch.equal(rots, hier.rotations)
    assert torch.equal(scales, hier.log_scales)  # log-scales, as save_hier passes them
    assert torch.equal(shs[:, :4], hier.shs) and not shs[:, 4:].any()
    assert torch.equal(nodes, hier.nodes) and torch.equal(boxes, hier.boxes)


def test_gpu_tolerances_are_four_times_the_float32_basis():
    """tests/test_gpu_hier_build.py's bounds are 4 x the recorded float32-against-float64 error of the
    numpy step on the GPU test's own cases, and the recorded values are what this machine measures
    (another LAPACK or libm may move them a little: within a factor of 1.5)."""
    import test_gpu_hier_build as G
    assert G.BOUNDS == {k: 4.0 * v for k, v in G.FP32_MEASURED.items()}
    now = R.fp32_basis()
    assert set(now) == set(G.FP32_MEASURED)
    for k, v in now.items():
        assert G.FP32_MEASURED[k] / 1.5 <= v <= G.FP32_MEASURED[k] * 1.5, (k, v, G.FP32_MEASURED[k])
