"""Cost of the hierarchy merger (gs_train.hier_merge, DESIGN.md "Hierarchy merger") on one GPU.

Two inputs: 8 chunks of a synthetic street chunk (gs_train.chunk.street_chunk: the hierarchy of the rows
after the skybox, 320k rows, repeated along the chunk's longest axis at 0.6 of its extent so that
neighbours overlap, each copy's attributes jittered) and 4 random frustum clouds of 5M rows whose
centres sit inside one another's clouds.  Each merge is repeated and the first is left out; the whole
merge_hierarchies call between two HIP events on the stream (its concatenation of the chunks, its
allocations and host reads included), the library's own per-stage split (gsr_hier_merge_stage_ms), the
gather stage's bytes -- per output node 268 B read and 268 B written (59 floats and the box) and the
8-B source entry -- over its time against the HBM rate, and the scratch bytes per input node.

    python tools/hier_merge_bench.py [--chunks 8] [--street-rows 300000] [--clouds 4] [--rows 5000000] [--reps 5]

Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "street-sparse-3dgs_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

HBM_TBPS = 8.0  # MI355X peak HBM rate


def med(v):
    return round(statistics.median(v), 3)


def time_merges(chunks, centres, reps):
    from gs_train.hier_merge import merge_hierarchies, scratch_bytes, stage_ms
    total, stages, m = [], [], None
    for k in range(reps + 1):
        del m
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m = merge_hierarchies(chunks, centres)
        e1.record()
        e1.synchronize()
        if k:  # the first merge is the warm-up
            total.append(e0.elapsed_time(e1))
            stages.append(stage_ms())
    T = sum(int(h.nodes.shape[0]) for h in chunks)
    N, M = int(m.nodes.shape[0]), int(m.shs.shape[1])
    st = {s: med([x[s] for x in stages]) for s in stages[0]}
    row = 4 * (11 + 3 * M + 8)
    gather_bytes = N * (2 * row + 8)
    return {"chunks": len(chunks), "input_nodes": T, "nodes": N, "leaves": list(m.chunk_leaves), "levels": m.levels, "M": M,
            "merge_ms": [round(t, 3) for t in total], "merge_ms_median": med(total), "stage_ms_median": st,
            "library_ms_median": round(sum(st.values()), 3), "gather_bytes": gather_bytes,
            "gather_TBps": round(gather_bytes / (st["gather"] * 1e-3) / 1e12, 3),
            "gather_share_of_hbm_peak": round(gather_bytes / (st["gather"] * 1e-3) / 1e12 / HBM_TBPS, 3),
            "scratch_bytes_per_input_node": round(scratch_bytes(len(chunks), T) / T, 2)}


def shifted(h, shift, seed):
    """A copy of hierarchy h moved by `shift`, its attributes jittered as another chunk's training would."""
    from gs_train.hier_build import Hierarchy
    g = torch.Generator(device=h.means3D.device).manual_seed(seed)
    n = lambda t, s: t + s * torch.randn(t.shape, generator=g, device=t.device)
    boxes = h.boxes.clone()
    boxes[:, :, :3] += shift
    return Hierarchy(n(h.means3D, 0.01) + shift, n(h.log_scales, 0.05), n(h.rotations, 0.02), h.opacities.clone(),
                     n(h.shs, 0.01), h.nodes, boxes, h.leaf_rows, h.levels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=8, help="copies of the street chunk (0: skip it)")
    ap.add_argument("--street-rows", type=int, default=300_000, help="LiDAR-like rows of the street chunk")
    ap.add_argument("--clouds", type=int, default=4, help="random clouds (0: skip them)")
    ap.add_argument("--rows", type=int, default=5_000_000, help="rows of each random cloud")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    from gs_train.hier_build import build_hierarchy
    out = {}
    if a.chunks:
        from gs_train.chunk import street_chunk
        from gs_train.native_step import NativeTrainStep
        torch.manual_seed(0)
        ts, info = street_chunk(NativeTrainStep, W=256, H=256, positions=2, n_init=a.street_rows, iterations=10, device=dev)
        g = ts.g
        with torch.no_grad():
            cols = [g._xyz.detach().clone(), g._scaling.detach().clone(), g._rotation.detach().clone(),
                    torch.sigmoid(g._opacity.detach()), g.get_features.detach().contiguous()]
        first = int(ts.skybox)
        del ts, g
        h = build_hierarchy(*cols, first_row=first)
        del cols
        lo, hi = h.means3D.min(0).values, h.means3D.max(0).values
        axis = int(torch.argmax(hi - lo))
        step = torch.zeros(3, device=dev)
        step[axis] = 0.6 * (hi - lo)[axis]
        chunks = [shifted(h, k * step, seed=k) for k in range(a.chunks)]
        centres = torch.stack([0.5 * (lo + hi) + k * step for k in range(a.chunks)]).cpu()
        out["street_chunks"] = dict(time_merges(chunks, centres, a.reps), rows_per_chunk=int((h.nodes.shape[0] + 1) // 2))
        del chunks, h
        torch.cuda.empty_cache()
    if a.clouds:
        from hier_build_bench import random_cloud
        chunks = []
        for k in range(a.clouds):
            chunks.append(build_hierarchy(*random_cloud(a.rows, dev, seed=k)))
        # the clouds share one frustum: centres spread across it give each chunk a wedge of every cloud
        centres = torch.tensor([[(-6.0 + 12.0 * k / max(a.clouds - 1, 1)), 0.0, 20.0] for k in range(a.clouds)])
        out["random_clouds"] = dict(time_merges(chunks, centres, a.reps), rows_per_chunk=a.rows)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
