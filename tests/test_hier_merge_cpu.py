"""CPU checks of the hierarchy merger's rule (DESIGN.md "Hierarchy merger") as restated in
tests/hier_merge_ref.py, the checker of csrc/hier_merge.hip, and of the merger's host surface: the
ctypes table against include/gsr_hier_merge.h and the library, the argument errors of the C entry
points and of gs_train.hier_merge without a GPU, read_centres, the command line's arguments and
load_chunk on a file with trailing skybox rows.

The gaussianhierarchy tool is not vendored in the reference, so parity against it is UNPINNED.  What is
pinned here, on the restatement over chunks from hier_build_ref.build (P <= 300): N = 2K - 1, the
breadth-first layout of DESIGN 14.1 C, every retained node named once by `source`, boxes nested along
every root path, and that the unchanged cut oracle (gso_expand_to_size) selects exactly one
ancestor-or-self of every surviving leaf."""
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
import hier_merge_ref as MR  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gsr_hier_merge.h")
ENTRY_POINTS = {"gsr_hier_merge_scratch_bytes", "gsr_hier_merge_top_floats", "gsr_hier_merge_plan",
                "gsr_hier_merge_gather", "gsr_hier_merge_stage_ms"}
SMALL = ["c1_p1", "c2_p64_p65", "c2_equidistant", "c2_one_empty", "nan_leaves", "c70_p300", "c_batch_plus_1"]
_merged = {}


def _case(name):
    if name not in _merged:
        chunks, centres = MR.cpu_case(name)
        _merged[name] = (chunks, centres, MR.merge(chunks, centres))
    return _merged[name]


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
    table = _lib.HIER_MERGE_SIGNATURES
    assert set(table) == set(decl), "ctypes table out of sync with include/gsr_hier_merge.h"
    for name, n in decl.items():
        assert len(table[name][1]) == n, f"{name}: {len(table[name][1])} ctypes arguments, the header has {n}"
    assert not set(table) & (set(_lib.SIGNATURES) | set(_lib.GT_SIGNATURES) | set(_lib.EVAL_SIGNATURES)
                             | set(_lib.HIER_BUILD_SIGNATURES))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), f"libgsr_hip.so does not export {name}"
    L = _lib.load()
    assert L.gsr_hier_merge_scratch_bytes.restype is ctypes.c_size_t
    assert L.gsr_abi_version() == _lib.ABI_VERSION  # new entry points only: the version stays
    from gs_train import hier_merge
    assert hier_merge.CENTRE_BATCH == MR.CENTRE_BATCH
    assert re.search(r"#define\s+GSR_HIER_MERGE_CENTRE_BATCH\s+%d\b" % MR.CENTRE_BATCH, open(HEADER).read())


def test_native_calls_validate_without_gpu():
    """Argument checks return before any device work."""
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    sb = L.gsr_hier_merge_scratch_bytes
    assert sb(0, 10) == 0 and sb(3, 2) == 0 and sb(1, 1 << 31) == 0
    need = sb(2, 1998)
    assert 0 < need < 1998 * 32 + (1 << 20) and sb(2, 4000) >= need
    assert L.gsr_hier_merge_top_floats(3, 16) == 5 * 67 and L.gsr_hier_merge_top_floats(0, 16) == 0
    one = ctypes.c_void_p(16)  # never dereferenced: the calls fail on their arguments
    first = (ctypes.c_int64 * 3)(0, 999, 1998)
    leaves = (ctypes.c_int64 * 2)()
    n_out, lv = ctypes.c_int64(5), ctypes.c_int(7)

    def plan(C=2, cf=first, M=16, dev=None, outs=None, scratch=one, nbytes=1 << 40, lv_=ctypes.byref(lv)):
        dev = [one] * 8 if dev is None else dev
        outs = [one] * 4 if outs is None else outs
        return L.gsr_hier_merge_plan(C, cf, M, *dev, leaves, ctypes.byref(n_out), lv_, *outs, scratch, nbytes, None)

    assert plan(C=0) == -1 and b"gsr_hier_merge" in L.gsr_last_error()
    for M in (0, 17):
        assert plan(M=M) == -1 and b"M must be" in L.gsr_last_error()
    for k in range(8):
        assert plan(dev=[one] * k + [None] + [one] * (7 - k)) == -1 and b"NULL" in L.gsr_last_error()
    for k in range(4):
        assert plan(outs=[one] * k + [None] + [one] * (3 - k)) == -1 and b"NULL" in L.gsr_last_error()
    assert plan(scratch=None) == -1 and plan(lv_=None) == -1 and plan(cf=None) == -1
    assert plan(cf=(ctypes.c_int64 * 3)(1, 999, 1998)) == -1 and b"start at 0" in L.gsr_last_error()
    assert plan(cf=(ctypes.c_int64 * 3)(0, 1000, 1999)) == -1 and b"chunk 0" in L.gsr_last_error()  # an even count
    assert plan(cf=(ctypes.c_int64 * 3)(0, 999, 999)) == -1 and b"chunk 1" in L.gsr_last_error()  # an empty chunk
    assert plan(cf=(ctypes.c_int64 * 3)(0, 1, 1 << 31)) == -1 and b"2^31" in L.gsr_last_error()
    assert plan(dev=[one] * 3 + [ctypes.c_void_p(20)] + [one] * 4) == -1 and b"aligned" in L.gsr_last_error()
    assert plan(nbytes=need - 1) == -1 and b"scratch too small" in L.gsr_last_error()
    assert n_out.value == 0 and lv.value == 0  # reset by every call

    def gather(C=2, M=16, N=5, p=None, scratch=one, nbytes=1 << 40):
        p = [one] * 15 if p is None else p
        return L.gsr_hier_merge_gather(C, M, N, *p, scratch, nbytes, None)

    assert gather(C=0) == -1 and gather(M=0) == -1 and gather(N=4) == -1 and gather(N=0) == -1
    for k in range(15):
        assert gather(p=[one] * k + [None] + [one] * (14 - k)) == -1 and b"NULL" in L.gsr_last_error()
    assert gather(scratch=None) == -1
    assert gather(p=[one] * 11 + [ctypes.c_void_p(4)] + [one] * 3) == -1 and b"aligned" in L.gsr_last_error()
    assert gather(nbytes=8) == -1 and b"scratch too small" in L.gsr_last_error()
    buf = (ctypes.c_float * 6)()
    assert L.gsr_hier_merge_stage_ms(buf, 6) == 6 and L.gsr_hier_merge_stage_ms(buf, 2) == 2
    assert L.gsr_hier_merge_stage_ms(None, 6) == 0


def _hier(ch):
    from gs_train.hier_build import Hierarchy
    t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a)).to(dt)
    nodes = t(ch["nodes"], torch.int32)
    return Hierarchy(t(ch["means3D"]), t(ch["log_scales"]), t(ch["rotations"]), t(ch["opacities"]), t(ch["shs"]), nodes,
                     t(ch["boxes"]), torch.where(nodes[:, 6] == 0, nodes[:, 2], -1).to(torch.int32),
                     int(ch["nodes"][:, 0].max()) + 1)


def test_merge_hierarchies_argument_errors_without_gpu():
    import dataclasses
    from gs_train.hier_merge import merge_hierarchies
    chunks, centres, _ = _case("c2_p64_p65")
    hs = [_hier(c) for c in chunks]
    cen = torch.from_numpy(centres)
    rep = lambda h, **kw: dataclasses.replace(h, **kw)
    with pytest.raises(TypeError):
        merge_hierarchies(hs[0], cen)
    with pytest.raises(TypeError):
        merge_hierarchies([hs[0], chunks[1]], cen)
    with pytest.raises(ValueError, match="at least one"):
        merge_hierarchies([], cen[:0])
    with pytest.raises(ValueError, match="centres"):
        merge_hierarchies(hs, cen[:1])
    with pytest.raises(ValueError, match="non-finite"):
        merge_hierarchies(hs, torch.tensor([[0.0, 0.0, float("nan")], [1.0, 0.0, 0.0]]))
    with pytest.raises(ValueError, match="chunk 1: nodes"):
        merge_hierarchies([hs[0], rep(hs[1], nodes=hs[1].nodes[:-1])], cen)  # an even node count
    with pytest.raises(ValueError, match="int32"):
        merge_hierarchies([rep(hs[0], nodes=hs[0].nodes.long()), hs[1]], cen)
    with pytest.raises(ValueError, match="means3D"):
        merge_hierarchies([rep(hs[0], means3D=hs[0].means3D[:-1]), hs[1]], cen)  # fewer rows than nodes
    with pytest.raises(ValueError, match="rotations"):
        merge_hierarchies([rep(hs[0], rotations=hs[0].rotations[:, :3]), hs[1]], cen)
    with pytest.raises(ValueError, match="shs"):
        merge_hierarchies([rep(hs[0], shs=torch.zeros(hs[0].shs.shape[0], 17, 3)), hs[1]], cen)
    with pytest.raises(ValueError, match="boxes"):
        merge_hierarchies([rep(hs[0], boxes=hs[0].boxes[:-1]), hs[1]], cen)
    with pytest.raises(ValueError, match="float32"):
        merge_hierarchies([rep(hs[0], log_scales=hs[0].log_scales.double()), hs[1]], cen)
    # valid arguments on the CPU: refused as not on a GPU (there is no CPU path)
    with pytest.raises(RuntimeError):
        merge_hierarchies(hs, cen)


def test_ownership_is_fp32_lowest_index_on_ties_and_never_non_finite():
    cen = np.array([[-1, 0, 10], [1, 0, 10], [-1, 0, 10]], np.float32)
    x = np.array([[0, 3, 4], [-0.5, 0, 0], [0.5, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [3e19, 0, 0]], np.float32)
    assert MR.owners(x, cen).tolist() == [0, 0, 1, -1, -1, -1]  # 3e19^2 overflows fp32: +inf never wins
    # the sum is (dx dx + dy dy) + dz dz in fp32, not float64 rounded once
    rng = np.random.default_rng(0)
    xs = rng.normal(0, 5, (4000, 3)).astype(np.float32)
    c2 = rng.normal(0, 5, (7, 3)).astype(np.float32)
    d = xs[:, None, :].astype(np.float32) - c2[None]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == np.float32 and np.array_equal(MR.owners(xs, c2), d2.argmin(1))


def test_validate_names_the_first_offending_node():
    chunks, _, _ = _case("c2_p64_p65")
    nodes = chunks[0]["nodes"]
    assert MR.validate(nodes) == -1
    for n, col, val in ((5, 1, 5), (9, 1, 40), (3, 2, 4), (0, 1, 0), (7, 0, 1)):
        bad = nodes.copy()
        bad[n, col] = val
        assert 0 <= MR.validate(bad) <= n
    inner = int(np.nonzero(nodes[:, 6] == 2)[0][3])
    bad = nodes.copy()
    bad[inner, 4] = 2  # count_merged
    assert MR.validate(bad) == inner
    bad = nodes.copy()
    bad[inner, 5] = nodes.shape[0] - 1  # the second child would lie past the chunk
    assert MR.validate(bad) <= inner
    with pytest.raises(ValueError, match="chunk 1: node"):
        MR.merge([chunks[0], dict(chunks[1], nodes=bad[:chunks[1]["nodes"].shape[0]])], np.zeros((2, 3), np.float32))


@pytest.mark.parametrize("name", SMALL)
def test_restatement_invariants(name):
    chunks, centres, m = _case(name)
    nodes, src, boxes = m["nodes"], m["source"], m["boxes"]
    K = sum(m["K_c"])
    N = 2 * K - 1
    assert nodes.shape == (N, 7) and nodes.dtype == np.int32 and m["levels"] == nodes[:, 0].max() + 1
    # the layout of DESIGN 14.1 C
    leaf = nodes[:, 6] == 0
    inner = np.nonzero(~leaf)[0]
    assert leaf.sum() == K
    assert np.array_equal(nodes[0, :2], (0, -1)) and np.array_equal(nodes[:, 2], np.arange(N))
    assert np.array_equal(nodes[leaf, 3:], np.tile((1, 0, -1, 0), (K, 1)))
    assert np.array_equal(nodes[inner, 3:5], np.tile((0, 1), (K - 1, 1)))
    assert (np.diff(nodes[:, 0]) >= 0).all()
    assert np.array_equal(nodes[inner, 5], 1 + 2 * np.arange(K - 1))
    ca = nodes[inner, 5]
    for k in (ca, ca + 1):
        assert np.array_equal(nodes[k, 1], inner) and np.array_equal(nodes[k, 0], nodes[inner, 0] + 1)
    assert MR.validate(nodes) == -1  # a merged hierarchy is itself in the builder's layout
    assert np.array_equal(m["leaf_rows"], np.where(leaf, src[:, 1], -1))
    # source: every retained node of every chunk exactly once, new top nodes {-1, -1}
    top = src[:, 0] < 0
    Ca = sum(k > 0 for k in m["K_c"])
    assert top.sum() == Ca - 1 and (src[top] == -1).all() and not leaf[top].any()
    for c, ch in enumerate(chunks):
        sel = np.nonzero(src[:, 0] == c)[0]
        own = MR.owners(ch["means3D"], centres) == c
        surv, kind, eff = MR.splice(ch["nodes"], own)
        assert m["K_c"][c] == int((kind == 1).sum()) and len(sel) == max(2 * m["K_c"][c] - 1, 0)
        assert sorted(src[sel, 1].tolist()) == np.nonzero(kind > 0)[0].tolist()
        assert np.array_equal(leaf[sel], kind[src[sel, 1]] == 1)
        # rows and boxes are copies, the opacity sign kept
        assert np.array_equal(m["means3D"][sel].astype(np.float32), ch["means3D"][src[sel, 1]], equal_nan=True)
        assert np.array_equal(m["opacities"][sel].astype(np.float32), ch["opacities"].reshape(-1)[src[sel, 1]])
        assert np.array_equal(boxes[sel], ch["boxes"][src[sel, 1]])
        # the new parent is the nearest retained strict ancestor, child order by old id
        old_parent = ch["nodes"][:, 1]
        for n in sel:
            p = old_parent[src[n, 1]]
            while p >= 0 and kind[p] != 2:
                p = old_parent[p]
            q = nodes[n, 1]
            if p >= 0:
                assert src[q, 0] == c and src[q, 1] == p
            else:
                assert q < 0 or src[q, 0] < 0  # the chunk's root hangs under the top tree
        a = src[ca, :]
        same = (a[:, 0] >= 0) & (a[:, 0] == src[ca + 1, 0]) & (src[inner, 0] >= 0)
        assert (a[same, 1] < src[ca + 1][same, 1]).all()
    if (src[:, 0] >= 0).any() and name != "nan_leaves":
        assert (np.asarray(m["opacities"])[src[:, 0] >= 0] < 0).any()  # perturb() left negative opacities
    # boxes nest along every root path, sizes are the largest extent
    for k in (ca, ca + 1):
        assert (boxes[k, 0, :3] >= boxes[inner, 0, :3]).all() and (boxes[k, 1, :3] <= boxes[inner, 1, :3]).all()
    assert np.array_equal(boxes[:, 0, 3], R.box_extent(boxes)) and not boxes[:, 1, 3].any()
    t = np.nonzero(top)[0]
    tc = nodes[t, 5]
    assert np.array_equal(boxes[t, 0, :3], np.minimum(boxes[tc, 0, :3], boxes[tc + 1, 0, :3]))
    assert np.array_equal(boxes[t, 1, :3], np.maximum(boxes[tc, 1, :3], boxes[tc + 1, 1, :3]))
    q = m["rotations"][t]
    assert np.allclose((q * q).sum(1), 1.0, atol=1e-12) and (m["opacities"][t] >= 0).all()
    assert np.isfinite(m["log_scales"][t]).all() and np.isfinite(m["means3D"][t]).all()


def test_cases_do_what_their_names_say():
    ch, cen, m = _case("c2_equidistant")
    for c in (0, 1):
        leaves = np.nonzero(ch[c]["nodes"][:, 6] == 0)[0]
        tied = leaves[ch[c]["means3D"][leaves, 0] == 0.0]
        assert len(tied) >= 20
        kept = set(m["source"][m["source"][:, 0] == c, 1].tolist())
        assert all((t in kept) == (c == 0) for t in tied.tolist())  # chunk 0 keeps them, chunk 1 drops them
    assert _case("c2_one_empty")[2]["K_c"] == [300, 0]
    ch, cen, m = _case("nan_leaves")
    for c in (0, 1):
        bad = np.nonzero(~np.isfinite(ch[c]["means3D"]).all(1) & (ch[c]["nodes"][:, 6] == 0))[0]
        assert len(bad) > 30 and not set(bad.tolist()) & set(m["source"][m["source"][:, 0] == c, 1].tolist())
    m = _case("c_batch_plus_1")[2]
    assert len(m["K_c"]) == MR.CENTRE_BATCH + 1 and m["K_c"][-1] > 0  # the chunk past the batch owns leaves
    m = _case("c70_p300")[2]
    top = m["source"][:, 0] < 0
    assert top.sum() == 69 and m["nodes"][top, 0].max() >= 6
    with pytest.raises(ValueError, match="no chunk has a surviving leaf"):
        MR.merge(*MR.cpu_case("all_nonfinite"))


def test_one_chunk_that_owns_everything_comes_back_unchanged():
    chunks, centres = MR.cpu_case("c1_p1000")
    m = MR.merge(chunks, centres)
    ch = chunks[0]
    assert np.array_equal(m["nodes"], ch["nodes"]) and np.array_equal(m["boxes"], ch["boxes"])
    assert np.array_equal(m["source"][:, 1], np.arange(1999)) and not m["source"][:, 0].any()
    for k in ("means3D", "log_scales", "rotations", "shs"):
        assert np.array_equal(m[k].astype(np.float32), ch[k])


VIEWPOINTS, targets, assert_cut_covers_each_leaf_once = MR.VIEWPOINTS, MR.targets, MR.assert_cut_covers_each_leaf_once


@pytest.mark.parametrize("name", ["c2_p64_p65", "nan_leaves", "c70_p300"])
def test_unchanged_cut_oracle_selects_one_ancestor_or_self_of_every_surviving_leaf(name):
    import gs_oracle as O
    _, _, m = _case(name)
    nodes, boxes = m["nodes"], m["boxes"]
    lengths = []
    for v in VIEWPOINTS:
        v = np.asarray(v, np.float32)
        for target in targets(boxes, v):
            ri, pi, ni = O.expand_to_size(nodes, boxes, target, v)
            assert_cut_covers_each_leaf_once(nodes, ni)
            assert np.array_equal(ri, ni)  # Gaussian row n belongs to node n
            lengths.append(len(ni))
        assert sorted(ni.tolist()) == np.nonzero(nodes[:, 6] == 0)[0].tolist()  # target 0: the leaves
    assert lengths[0] < lengths[2]


def test_read_centres_and_the_command_line(tmp_path):
    from gs_train import hier_merge as HM
    for name, text in (("0_0", "1.5 -2 3e1\n"), ("0_1", " 4\t5\n6 ")):
        os.makedirs(tmp_path / "chunks" / name)
        (tmp_path / "chunks" / name / "center.txt").write_text(text)
    cen = HM.read_centres(str(tmp_path / "chunks"), ["0_1", "0_0"])
    assert cen.dtype == torch.float32 and cen.tolist() == [[4.0, 5.0, 6.0], [1.5, -2.0, 30.0]]
    (tmp_path / "chunks" / "0_0" / "center.txt").write_text("1 2\n")
    with pytest.raises(ValueError, match="three numbers"):
        HM.read_centres(str(tmp_path / "chunks"), ["0_0"])
    (tmp_path / "chunks" / "0_0" / "center.txt").write_text("1 2 x\n")
    with pytest.raises(ValueError, match="not numbers"):
        HM.read_centres(str(tmp_path / "chunks"), ["0_0"])
    with pytest.raises(FileNotFoundError):
        HM.read_centres(str(tmp_path / "chunks"), ["9_9"])
    # <trained_chunks> <skybox_points> <chunks_dir> <out.hier> <chunk>...
    assert HM.parse_args(["tr", "0", "ch", "out.hier", "0_0", "0_1"]) == ("tr", "ch", "out.hier", ["0_0", "0_1"])
    with pytest.raises(ValueError, match="usage"):
        HM.parse_args(["tr", "0", "ch", "out.hier"])
    with pytest.raises(ValueError, match="skybox_points other than 0"):
        HM.parse_args(["tr", "100", "ch", "out.hier", "0_0"])
    with pytest.raises(ValueError, match="integer"):
        HM.parse_args(["tr", "many", "ch", "out.hier", "0_0"])
    # every argument error comes before any device work: a missing chunk file too
    (tmp_path / "chunks" / "0_0" / "center.txt").write_text("1 2 3\n")
    with pytest.raises(FileNotFoundError, match="hierarchy.hier_opt"):
        HM.main([str(tmp_path / "trained"), "0", str(tmp_path / "chunks"), str(tmp_path / "merged.hier"), "0_0"])


def test_load_chunk_drops_the_skybox_rows_after_the_nodes(tmp_path):
    from gaussian_hierarchy._C import write_hierarchy
    from gs_train.hier_merge import load_chunk
    chunks, _, _ = _case("c2_p64_p65")
    h = _hier(chunks[0])
    N, S = h.nodes.shape[0], 11
    g = torch.Generator().manual_seed(0)
    sky = lambda *s: torch.rand(*s, generator=g)
    path = str(tmp_path / "hierarchy.hier_opt")  # as save_hier writes it: N node rows, then the skybox rows
    write_hierarchy(path, torch.cat([h.means3D, sky(S, 3)]), torch.cat([h._shs16(), sky(S, 16, 3)]),
                    torch.cat([h.opacities, sky(S, 1)]), torch.cat([h.log_scales, sky(S, 3)]),
                    torch.cat([h.rotations, sky(S, 4)]), h.nodes, h.boxes)
    got = load_chunk(path, "cpu")
    assert got.means3D.shape == (N, 3) and got.shs.shape == (N, 16, 3) and got.opacities.shape == (N, 1)
    assert torch.equal(got.means3D, h.means3D) and torch.equal(got.opacities, h.opacities)
    assert torch.equal(got.shs[:, :h.shs.shape[1]], h.shs) and torch.equal(got.nodes, h.nodes)
    assert torch.equal(got.boxes, h.boxes) and torch.equal(got.leaf_rows, h.leaf_rows) and got.levels == h.levels
    with open(path, "r+b") as f:  # a negative row count marks the compressed variant
        f.write(np.int32(-(N + S)).tobytes())
    with pytest.raises(NotImplementedError, match="compressed"):
        load_chunk(path, "cpu")
    write_hierarchy(path, h.means3D[:-1], h._shs16()[:-1], h.opacities[:-1], h.log_scales[:-1], h.rotations[:-1], h.nodes,
                    h.boxes)
    with pytest.raises(ValueError, match="one Gaussian per node"):
        load_chunk(path, "cpu")


def test_gpu_tolerances_are_four_times_the_float32_basis():
    """tests/test_gpu_hier_merge.py's bounds are 4 x the recorded float32-against-float64 error of the
    numpy step on the GPU test's own top-tree steps, and the recorded values are what this machine
    measures (another LAPACK or libm may move them a little: within a factor of 1.5)."""
    import test_gpu_hier_merge as G
    assert G.BOUNDS == {k: 4.0 * v for k, v in G.FP32_MEASURED.items()}
    now = MR.fp32_basis()
    assert set(now) == set(G.FP32_MEASURED)
    for k, v in now.items():
        assert G.FP32_MEASURED[k] / 1.5 <= v <= G.FP32_MEASURED[k] * 1.5, (k, v, G.FP32_MEASURED[k])
