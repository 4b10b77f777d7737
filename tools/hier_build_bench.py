"""Cost of the LOD hierarchy builder (gs_train.hier_build, DESIGN.md "Hierarchy builder") on one GPU.

Builds the hierarchy of a synthetic street chunk's Gaussians (gs_train.chunk.street_chunk: the rows
after the skybox) and of random frustum clouds (default 1M and 5M rows): each build is repeated and the
first is left out; the whole build between two HIP events on the stream, the library's own per-stage
split (sort / topology / numbering / merge, gsr_hier_build_stage_ms), the level count and the scratch
bytes per row.

    python tools/hier_build_bench.py [--rows 1000000 5000000] [--street-rows 300000] [--reps 5]

Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "street-sparse-3dgs_amd"))

import torch  # noqa: E402


def med(v):
    return round(statistics.median(v), 3)


def time_builds(cols, first_row, reps):
    from gs_train._native import lib
    from gs_train.hier_build import build_hierarchy, stage_ms
    total, stages, h = [], [], None
    for k in range(reps + 1):
        del h
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        h = build_hierarchy(*cols, first_row=first_row)
        e1.record()
        e1.synchronize()
        if k:  # the first build is the warm-up
            total.append(e0.elapsed_time(e1))
            stages.append(stage_ms())
    P = cols[0].shape[0] - first_row
    return {"rows": P, "nodes": int(h.nodes.shape[0]), "levels": h.levels, "M": int(cols[4].shape[1]),
            "build_ms": [round(t, 3) for t in total], "build_ms_median": med(total),
            "stage_ms_median": {s: med([x[s] for x in stages]) for s in stages[0]},
            "scratch_bytes_per_row": round(lib().gsr_hier_build_scratch_bytes(P) / P, 2)}


def random_cloud(P, dev, seed=0):
    from gs_train.synthetic import camera
    g = torch.Generator(device=dev).manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, device=dev)
    _, _, _, tx, ty = camera(1920, 1080)
    z = 2.0 + 38.0 * u(P)
    xyz = torch.stack([(u(P) * 1.9 - 0.95) * tx * z, (u(P) * 1.9 - 0.95) * ty * z, z], 1).contiguous()
    ls = -4.5 + 0.5 * torch.randn(P, 3, generator=g, device=dev)
    q = torch.randn(P, 4, generator=g, device=dev)
    shs = 0.05 * torch.randn(P, 16, 3, generator=g, device=dev)
    return xyz, ls, q, 0.05 + 0.94 * u(P, 1), shs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[1_000_000, 5_000_000])
    ap.add_argument("--street-rows", type=int, default=300_000, help="LiDAR-like rows of the street chunk (0: skip it)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = {}
    if a.street_rows:
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
        out["street_chunk"] = dict(time_builds(cols, first, a.reps), skybox_rows=first)
        del cols
    for P in a.rows:
        out[f"random_{P}"] = time_builds(random_cloud(P, dev), 0, a.reps)
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
