"""One station's six faces two ways, interleaved in one process (measurement tool, run on the GPU box):

  (a) six single-view fused cut frames, each with its own expand_to_size and
      get_interpolation_weights -- the reference's order of work (render_hierarchy.py draws every
      camera on its own);
  (b) one gs_train.station.StationRenderer.render call.

The scene is a shell hierarchy (synthetic_lod_hierarchy(layout="shell")) of config 5's size by
default (37.5M leaves, 100 000 skybox rows) around the station, the faces 1024 x 1024 with tanfov 1,
tau 15 px.  Pre-warmed, then `--rounds` rounds of (a), (b) in alternating order; per-station wall
time after a device sync (both paths wait on the host for their counts), median and p10-p90.  Then
`--rounds` profiled station calls for the stages' device times (HIP events): station_rows' own time
and its achieved bytes/s against the row bytes it must move.  Output: one JSON line, then a
readable summary."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "street-sparse-3dgs_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=37_500_000)
    ap.add_argument("--skybox", type=int, default=100_000)
    ap.add_argument("--face", type=int, default=1024)
    ap.add_argument("--faces", type=int, default=6, choices=(4, 6))
    ap.add_argument("--tau", type=float, default=15.0)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log-scale-mean", type=float, default=-6.0)
    a = ap.parse_args()

    import numpy as np
    import torch
    from diff_gaussian_rasterization import _C
    from gaussian_hierarchy._C import expand_to_size, get_interpolation_weights
    from gs_train import station as ST
    from gs_train.synthetic import cube_face_cameras, synthetic_lod_hierarchy, tau_threshold
    dev = torch.device("cuda:0")
    W = a.face
    h = synthetic_lod_hierarchy(a.leaves, W, W, dev, seed=5, skybox=a.skybox, log_scale_mean=a.log_scale_mean,
                                layout="shell")
    cams = cube_face_cameras(W, a.faces)
    N, Nn, S = h["means3D"].shape[0], h["nodes"].shape[0], a.skybox
    thr = float(np.float32(tau_threshold(a.tau, 1.0, W)))
    t = lambda x: torch.tensor(np.asarray(x), dtype=torch.float32, device=dev)
    bg = t([0.1, 0.2, 0.3])
    e = torch.empty(0, device=dev)
    ri, pi, ni = (torch.zeros(Nn + S, dtype=torch.int32, device=dev) for _ in range(3))
    w = torch.zeros(Nn + S, device=dev)
    k = torch.zeros(Nn + S, dtype=torch.int32, device=dev)
    sky = torch.arange(N - S, N, dtype=torch.int32, device=dev)
    z3 = torch.zeros(3)
    mats = [(t(c["view"]).reshape(4, 4), t(c["proj"]).reshape(4, 4), t(c["campos"])) for c in cams]

    def path_a():
        outs, R = [], 0
        with torch.no_grad():
            for view, proj, campos in mats:
                n = expand_to_size(h["nodes"], h["boxes"], thr, campos, z3, ri[:Nn], pi[:Nn], ni[:Nn])
                get_interpolation_weights(ni[:n], thr, h["nodes"], h["boxes"], campos.cpu(), z3, w, k)
                ri[n:n + S] = sky
                pi[n:n + S] = sky
                w[n:n + S] = 1.0
                R = n + S
                o = _C.rasterize_gaussians(bg, h["means3D"], e, h["opacities"], h["scales"], h["rotations"], 1.0, e,
                                           view, proj, 1.0, 1.0, W, W, h["shs"], 3, campos, False, False, ri[:R],
                                           pi[:R], w[:R], k[:R], True, need_backward=False)
                outs.append((o[0], o[1], o[2], o[3]))
        return outs, R

    sr = ST.StationRenderer(h, dev)

    def path_b():
        return sr.render(cams, a.tau, bg=(0.1, 0.2, 0.3))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(a.warmup):
        path_a()
        path_b()
    (ms, (ya, R)), (_, yb) = timed(path_a), timed(path_b)
    same = all(int(ya[f][0]) == sr.last_K[f] and torch.equal(ya[f][1], yb[0][f]) and torch.equal(ya[f][2], yb[1][f])
               and torch.equal(ya[f][3], yb[2][f]) for f in range(a.faces))
    kept, K = list(sr.last_kept), list(sr.last_K)
    ta, tb = [], []
    for r in range(a.rounds):
        order = (("a", path_a), ("b", path_b)) if r % 2 == 0 else (("b", path_b), ("a", path_a))
        for name, fn in order:
            (ta if name == "a" else tb).append(timed(fn)[0])
    ST.set_profiling(True)
    stages = []
    for _ in range(a.rounds):
        path_b()
        torch.cuda.synchronize()
        stages.append(ST.stage_times_ms())
    ST.set_profiling(False)
    med = lambda xs: float(np.median(xs))
    q = lambda xs, p: float(np.percentile(xs, p))
    st = {s: med([x[s] for x in stages]) for s in ST.STAGES}
    # station_rows: per row two gathered source rows (means 12, scales 12, rotation 16, opacity 4,
    # SH 192 B), the cut's 12 B, the staged row 52 B and its flag byte
    row_bytes = 2 * (12 + 12 + 16 + 4 + 192) + 12 + 52 + 1
    rows_ms = st["station_rows"]
    res = dict(leaves=a.leaves, nodes=int(Nn), skybox=S, face=W, faces=a.faces, tau=a.tau, cut_rows=int(R),
               rows_kept=kept, tile_instances=K, rounds=a.rounds, bitwise_equal=bool(same),
               a_six_frames_ms=dict(median=med(ta), p10=q(ta, 10), p90=q(ta, 90)),
               b_station_ms=dict(median=med(tb), p10=q(tb, 10), p90=q(tb, 90)),
               ratio_a_over_b=med(ta) / med(tb), station_stage_ms=st, row_bytes=row_bytes,
               station_rows_GBps=(row_bytes * R / (rows_ms * 1e-3) / 1e9) if rows_ms > 0 else None)
    print(json.dumps(res))
    print(f"cut {R} rows; faces keep {kept} ({sum(kept) / max(R, 1):.2f} x the cut in all)")
    print(f"(a) six single-view frames: {med(ta):.3f} ms per station (p10 {q(ta, 10):.3f}, p90 {q(ta, 90):.3f})")
    print(f"(b) one station call:       {med(tb):.3f} ms per station (p10 {q(tb, 10):.3f}, p90 {q(tb, 90):.3f})")
    print(f"ratio (a) / (b): {med(ta) / med(tb):.2f}; outputs bitwise equal: {same}")
    print("station stages (device ms, median): " + ", ".join(f"{s} {v:.3f}" for s, v in st.items()))
    if rows_ms > 0:
        print(f"station_rows: {row_bytes} B per row x {R} rows in {rows_ms:.3f} ms = "
              f"{row_bytes * R / (rows_ms * 1e-3) / 1e9:.0f} GB/s")


if __name__ == "__main__":
    main()
