"""Cost of a chunk's depth supervision maps on one GPU, stage by stage.

The synthetic street block of tools/lidar_prep_bench.py -- a ground strip and two facades meshed with
jittered triangles of about 0.35 m, four 50 m triangles under the block -- seen by `--cameras` pinhole
cameras that drive along the street 1.8 m above the ground, looking ahead and a little to either
side, at `--size` x `--size` pixels with fx = fy = size / 2.

  1. bin:    camera records, counts, scan, fill and sort of the (camera, tile, triangle) references,
             the call's one wait on the host (for their number) and its allocation included
  2. cast:   the ray cast kernel
  3. encode: gsr_depth_encode of the maps (quantised): three launches and the copy of scale / offset
1 and 2 are the microseconds gsr_mesh_distance_maps reports from device events it records on the
stream around the two stages (`stats`); the whole call and the encode are timed from here.
Device events around each call after `--warmup` calls, `--reps` repeats, median and minimum; the call
synchronises the stream, so an event pair measures what a caller waits for.  Reported with them: tile
references per triangle, the oversize list, the longest run a tile walks, rays per second, and with
--cpu the float64 reference (tests/mesh_depth_ref.cast64) on a 64 x 64 crop of one camera, with the
number of pixels on which the two differ in hit / miss or by more than the test's bar.

    python tools/mesh_depth_bench.py [--cameras 256] [--size 512] [--length 100] [--pitch 0.35] [--cpu]

Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "street-sparse-3dgs_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lidar_prep_bench import WIDTH, street_mesh  # noqa: E402


def street_cameras(n, length, size):
    """(n, 11): along the street's axis at 1.8 m, heading down it with a yaw sweeping +-35 degrees."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from mesh_depth_cases import look_at
    f = size / 2.0
    rows = []
    for k in range(n):
        x = 2.0 + (length - 30.0) * k / max(n - 1, 1)
        yaw = np.radians(35.0) * np.sin(k * 0.7)
        eye = np.array([x, WIDTH / 2 + 2.0 * np.sin(k * 0.31), 1.8])
        rows.append(look_at(eye, eye + [np.cos(yaw), np.sin(yaw), -0.05], f, f, size / 2.0, size / 2.0))
    return np.stack(rows)


def timed(fn, warmup, reps):
    ms = []
    for rep in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        if rep >= warmup:
            ms.append(e0.elapsed_time(e1))
    return out, ms


def summary(ms):
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=256)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--length", type=float, default=100.0)
    ap.add_argument("--pitch", type=float, default=0.35)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cpu", action="store_true", help="also run the float64 reference on a 64 x 64 crop of one camera")
    a = ap.parse_args()
    from gs_train import mesh_depth as M
    dev = torch.device("cuda")
    vertices, faces = street_mesh(a.length, a.pitch)
    cams = street_cameras(a.cameras, a.length, a.size)
    v_d, f_d = torch.tensor(vertices, device=dev), torch.tensor(faces, device=dev)
    q, t, k = cams[:, :4], cams[:, 4:7], cams[:, 7:]
    S, K, F = a.size, a.cameras, len(faces)
    out = {"cameras": K, "size": S, "vertices": len(vertices), "triangles": F, "device": torch.cuda.get_device_name(0)}

    st = {}
    full = lambda: M.render_mesh_distance(v_d, f_d, q, t, k, S, S, stats=st)
    dist, ms_full = timed(full, a.warmup, a.reps)
    bin_ms, cast_ms = [], []
    for _ in range(a.reps):
        full()
        bin_ms.append(st["bin_us"] / 1e3)
        cast_ms.append(st["cast_us"] / 1e3)
    rays = K * S * S
    m = statistics.median(ms_full)
    out["call"] = dict(summary(ms_full), rays_per_s=round(rays / (m * 1e-3)), references=st["references"],
                       references_per_triangle=round(st["references"] / (K * F), 3), oversize=st["oversize"],
                       oversize_per_camera=round(st["oversize"] / K, 1), longest_run=st["longest_run"],
                       occupied_tiles=st["occupied_tiles"], tiles=K * ((S + 15) // 16) ** 2,
                       references_per_occupied_tile=round(st["references"] / max(st["occupied_tiles"], 1), 1),
                       hit_fraction=round(float((dist > 0).float().mean()), 4))
    out["bin"] = dict(summary(bin_ms), references_per_s=round(st["references"] / (statistics.median(bin_ms) * 1e-3)))
    out["cast"] = dict(summary(cast_ms), rays_per_s=round(rays / (statistics.median(cast_ms) * 1e-3)))

    enc, ms_enc = timed(lambda: M.encode_depth_maps(dist), a.warmup, a.reps)
    m = statistics.median(ms_enc)
    out["encode"] = dict(summary(ms_enc), pixels_per_s=round(rays / (m * 1e-3)),
                         GBps_of_min=round(rays * (4 + 4 + 2) / (m * 1e-3) / 1e9, 1),
                         images_with_depth=int((enc.scale > 0).sum()))

    if a.cpu:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import mesh_depth_ref as R
        kc, n = K // 2, 64
        cam = cams[kc].copy()
        o = (S - n) // 2
        cam[9] -= o  # the crop's principal point
        cam[10] -= o
        t0 = time.perf_counter()
        r = R.cast64(vertices, faces, cam, n, n)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        got = dist[kc, o:o + n, o:o + n].cpu().numpy()
        with open(os.path.join(REPO, "profiles", "r20_mesh_depth_margins.jsonl")) as f:
            bar = 4.0 * [json.loads(ln)["units"] for ln in f if '"cpu_f32_worst"' in ln][0]
        bad = R.judge(got, r, bar)
        dec = ~r["boundary"]
        differ = int((dec & ((got > 0) != (r["distance"] > 0))).sum())
        hit = dec & (got > 0) & (r["distance"] > 0)
        over = int((np.abs(got - r["distance"])[hit] > bar * r["scale"][hit]).sum())
        out["cpu"] = {"camera": kc, "crop": n, "ms": round(cpu_ms, 1), "rays_per_s": round(n * n / (cpu_ms * 1e-3)),
                      "boundary_pixels": int(r["boundary"].sum()), "decided_hit_miss_differs": differ,
                      "decided_over_the_bar": over, "judge_problems": len(bad)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
