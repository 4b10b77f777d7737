"""merge_hierarchies: trained chunk hierarchies into one scene hierarchy on the device
(include/gsr_hier_merge.h, csrc/hier_merge.hip) -- the pipeline's last stage, which the reference runs
as the GaussianHierarchyMerger tool over every chunk's hierarchy.hier_opt (scripts/full_train.py:259-282)
to write the merged.hier render_hierarchy.py loads:

    chunks = [load_chunk(f"{trained}/{name}/hierarchy.hier_opt", "cuda") for name in names]
    merged = merge_hierarchies(chunks, read_centres(chunks_dir, names))
    merged.save(out_path)             # or merged.to_model(...)

    python -m gs_train.hier_merge <trained_chunks> 0 <chunks_dir> <out.hier> <chunk>...

Each chunk keeps the leaves nearer to its own centre than to any other chunk's, interior nodes left
with one surviving child are spliced out, and the chunk trees are joined under a new upper tree made
with the builder's own order, topology and merge step.  The rule (DESIGN.md "Hierarchy merger") is this
project's definition -- the published method's consolidation restated -- and is parity-unpinned against
the un-vendored gaussianhierarchy tool.  Not covered: anchors.bin, the compressed .hier variant.  There
is no CPU path.
"""
from __future__ import annotations

import ctypes
import os
import sys
from dataclasses import dataclass

import torch

from ._native import check, lib, ptr, require_gpu, stream
from .hier_build import Hierarchy

MAX_NODES = (1 << 31) - 1
CENTRE_BATCH = 256  # GSR_HIER_MERGE_CENTRE_BATCH
STAGES = ("ownership", "survive", "splice", "numbering", "top", "gather")


@dataclass
class MergedHierarchy(Hierarchy):
    """A Hierarchy of N = 2K - 1 rows whose leaf_rows[n] is a leaf's old node id in its chunk (-1 for
    an interior node), with source (N,2) int32 = {chunk, old node id} ({-1, -1} for a new top node)
    and chunk_leaves (C) = each chunk's surviving leaves."""
    source: torch.Tensor = None
    chunk_leaves: tuple = ()


def _check_chunks(chunks, centres):
    if isinstance(chunks, Hierarchy) or not hasattr(chunks, "__len__"):
        raise TypeError("merge_hierarchies: chunks must be a sequence of Hierarchy objects")
    if len(chunks) < 1:
        raise ValueError("merge_hierarchies: at least one chunk")
    for i, h in enumerate(chunks):
        if not isinstance(h, Hierarchy):
            raise TypeError(f"merge_hierarchies: chunk {i} must be a Hierarchy")
        N = h.nodes.shape[0] if h.nodes.dim() == 2 else -1
        if h.nodes.dim() != 2 or h.nodes.shape[1] != 7 or N < 1 or N % 2 == 0:
            raise ValueError(f"merge_hierarchies: chunk {i}: nodes must be (N, 7) with N = 2 P - 1")
        if h.nodes.dtype != torch.int32:
            raise ValueError(f"merge_hierarchies: chunk {i}: nodes must be int32")
        if h.means3D.dim() != 2 or h.means3D.shape[1] != 3 or h.means3D.shape[0] < N:
            raise ValueError(f"merge_hierarchies: chunk {i}: means3D must be (>= N, 3)")
        R = h.means3D.shape[0]
        if tuple(h.log_scales.shape) != (R, 3) or tuple(h.rotations.shape) != (R, 4):
            raise ValueError(f"merge_hierarchies: chunk {i}: log_scales must be (R, 3) and rotations (R, 4)")
        if tuple(h.opacities.shape) not in ((R, 1), (R,)):
            raise ValueError(f"merge_hierarchies: chunk {i}: opacities must be (R, 1) or (R,)")
        if h.shs.dim() != 3 or h.shs.shape[0] != R or h.shs.shape[2] != 3 or not 1 <= h.shs.shape[1] <= 16:
            raise ValueError(f"merge_hierarchies: chunk {i}: shs must be (R, M, 3) with 1 <= M <= 16")
        if tuple(h.boxes.shape) != (N, 2, 4):
            raise ValueError(f"merge_hierarchies: chunk {i}: boxes must be (N, 2, 4)")
        for t, n in ((h.means3D, "means3D"), (h.log_scales, "log_scales"), (h.rotations, "rotations"),
                     (h.opacities, "opacities"), (h.shs, "shs"), (h.boxes, "boxes")):
            if t.dtype != torch.float32:
                raise ValueError(f"merge_hierarchies: chunk {i}: {n} must be float32")
    if sum(h.nodes.shape[0] for h in chunks) > MAX_NODES:
        raise ValueError("merge_hierarchies: more than 2^31 - 1 nodes")
    centres = torch.as_tensor(centres)
    if tuple(centres.shape) != (len(chunks), 3):
        raise ValueError("merge_hierarchies: centres must be (C, 3), one per chunk")
    if not bool(torch.isfinite(centres.double()).all()):
        raise ValueError("merge_hierarchies: centres has non-finite values")
    return centres


def merge_hierarchies(chunks, centres):
    """chunks: a sequence of Hierarchy objects on one ROCm device, in the builder's layout, their
    attributes as train_post left them (rows past a chunk's N nodes -- the skybox -- are ignored; SH is
    zero-padded to the largest M).  centres (C,3): each chunk's centre.  Returns a MergedHierarchy.
    A chunk whose nodes break the layout is refused before anything follows its indices."""
    centres = _check_chunks(chunks, centres)
    tensors = [t for h in chunks for t in (h.means3D, h.log_scales, h.rotations, h.opacities, h.shs, h.nodes, h.boxes)]
    require_gpu(*tensors)
    dev = chunks[0].means3D.device
    if any(t.device != dev for t in tensors):
        raise RuntimeError("merge_hierarchies: the chunks must be on one device")
    C = len(chunks)
    M = max(h.shs.shape[1] for h in chunks)
    Ns = [h.nodes.shape[0] for h in chunks]
    first = [0]
    for n in Ns:
        first.append(first[-1] + n)
    T = first[-1]

    def shs_of(h, n):
        s = h.shs.detach()[:n]
        if s.shape[1] == M:
            return s
        out = torch.zeros(n, M, 3, dtype=torch.float32, device=dev)
        out[:, :s.shape[1]] = s
        return out

    cat = lambda f: torch.cat([f(h, n) for h, n in zip(chunks, Ns)]).contiguous()
    xyz = cat(lambda h, n: h.means3D.detach()[:n])
    ls = cat(lambda h, n: h.log_scales.detach()[:n])
    rot = cat(lambda h, n: h.rotations.detach()[:n])
    op = cat(lambda h, n: h.opacities.detach()[:n].reshape(n))
    shs = cat(shs_of)
    nodes = cat(lambda h, n: h.nodes)
    boxes = cat(lambda h, n: h.boxes.detach())
    cen = centres.to(device=dev, dtype=torch.float32).contiguous()

    L = lib()
    cap = T + C - 1
    nodes_out = torch.empty(cap, 7, dtype=torch.int32, device=dev)
    source = torch.empty(cap, 2, dtype=torch.int32, device=dev)
    top_rows = torch.empty(int(L.gsr_hier_merge_top_floats(C, M)), dtype=torch.float32, device=dev)
    top_node = torch.empty(2 * C - 1, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(L.gsr_hier_merge_scratch_bytes(C, T)), dtype=torch.uint8, device=dev)
    cfirst = (ctypes.c_int64 * (C + 1))(*first)
    leaves = (ctypes.c_int64 * C)()
    n_out, levels = ctypes.c_int64(0), ctypes.c_int(0)
    ins = [ptr(t) for t in (xyz, ls, rot, op, shs)]
    with torch.cuda.device(dev):
        check(L.gsr_hier_merge_plan(C, cfirst, M, ptr(cen), *ins, ptr(nodes), ptr(boxes), leaves, ctypes.byref(n_out),
                                    ctypes.byref(levels), ptr(nodes_out), ptr(source), ptr(top_rows), ptr(top_node),
                                    ptr(scratch), scratch.numel(), stream(dev)), "gsr_hier_merge_plan")
        N = int(n_out.value)
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        out = [f(N, 3), f(N, 3), f(N, 4), f(N, 1), f(N, M, 3)]
        out_boxes = f(N, 2, 4)
        check(L.gsr_hier_merge_gather(C, M, N, *ins, ptr(boxes), ptr(source), ptr(top_rows), ptr(top_node),
                                      *[ptr(t) for t in out], ptr(out_boxes), ptr(scratch), scratch.numel(), stream(dev)),
              "gsr_hier_merge_gather")
    nodes_out, source = nodes_out[:N].clone(), source[:N].clone()
    leaf_rows = torch.where(nodes_out[:, 6] == 0, source[:, 1], torch.full_like(source[:, 1], -1))
    return MergedHierarchy(*out, nodes_out, out_boxes, leaf_rows, int(levels.value), source, tuple(int(k) for k in leaves))


def stage_ms():
    """Device time of this thread's last merge in ms, by stage."""
    buf = (ctypes.c_float * 6)()
    n = lib().gsr_hier_merge_stage_ms(buf, 6)
    return dict(zip(STAGES, list(buf)[:n]))


def scratch_bytes(C, total_nodes):
    return int(lib().gsr_hier_merge_scratch_bytes(C, total_nodes))


def load_chunk(path, device):
    """A chunk's .hier / .hier_opt file as a Hierarchy on `device`.  save_hier also writes the skybox
    rows create_from_hier appended, so the file may hold more Gaussian rows than nodes: the rows past N
    are dropped.  The compressed variant fails loudly, as load_hierarchy does."""
    from gaussian_hierarchy._C import load_hierarchy
    xyz, shs, alpha, ls, rot, nodes, boxes = load_hierarchy(path)
    N = nodes.shape[0]
    if N < 1 or N % 2 == 0 or xyz.shape[0] < N or boxes.shape[0] != N:
        raise ValueError(f"load_chunk: {path}: {N} nodes, {xyz.shape[0]} Gaussian rows and {boxes.shape[0]} boxes are "
                         f"not a hierarchy of one Gaussian per node")
    d = lambda t: t.to(device)
    leaf_rows = torch.where(nodes[:, 6] == 0, nodes[:, 2], torch.full_like(nodes[:, 2], -1))
    levels = int(nodes[:, 0].max()) + 1
    return Hierarchy(d(xyz[:N].contiguous()), d(ls[:N].contiguous()), d(rot[:N].contiguous()),
                     d(alpha[:N].reshape(N, 1).contiguous()), d(shs[:N].contiguous()), d(nodes), d(boxes), d(leaf_rows), levels)


def read_centres(chunks_dir, names):
    """(C,3) float32: each <chunks_dir>/<name>/center.txt, three whitespace-separated numbers
    (preprocess/make_chunk.py:244-245 writes them)."""
    rows = []
    for name in names:
        path = os.path.join(chunks_dir, name, "center.txt")
        with open(path) as f:
            vals = f.read().split()
        if len(vals) != 3:
            raise ValueError(f"read_centres: {path}: expected three numbers, found {len(vals)}")
        try:
            rows.append([float(v) for v in vals])
        except ValueError:
            raise ValueError(f"read_centres: {path}: not numbers: {' '.join(vals)}") from None
    return torch.tensor(rows, dtype=torch.float32).reshape(len(rows), 3)


def parse_args(argv):
    """The merger's own argument order (scripts/full_train.py:263-268): <trained_chunks> <skybox_points>
    <chunks_dir> <out.hier> <chunk>...  Returns (trained_chunks, chunks_dir, out_path, chunk names)."""
    if len(argv) < 5:
        raise ValueError("hier_merge: usage: <trained_chunks> <skybox_points> <chunks_dir> <out.hier> <chunk>...")
    trained, sky, chunks_dir, out_path = argv[:4]
    try:
        sky = int(sky)
    except ValueError:
        raise ValueError(f"hier_merge: skybox_points must be an integer, not {sky!r}") from None
    if sky != 0:
        raise ValueError("hier_merge: skybox_points other than 0 is not supported (the pipeline always passes 0)")
    return trained, chunks_dir, out_path, list(argv[4:])


def main(argv=None, device="cuda"):
    trained, chunks_dir, out_path, names = parse_args(sys.argv[1:] if argv is None else list(argv))
    centres = read_centres(chunks_dir, names)
    paths = [os.path.join(trained, n, "hierarchy.hier_opt") for n in names]
    for p in paths:
        if not os.path.isfile(p):
            raise FileNotFoundError(f"hier_merge: {p} not found")
    chunks = [load_chunk(p, device) for p in paths]
    merged = merge_hierarchies(chunks, centres)
    merged.save(out_path)
    print(f"hier_merge: {len(names)} chunks, {sum(merged.chunk_leaves)} leaves, {merged.nodes.shape[0]} nodes, "
          f"{merged.levels} levels -> {out_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
