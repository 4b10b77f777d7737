"""Cost of the ground-truth cloud constraint of densification on one GPU.

  1. index build: GtPointCloud over a synthetic street cloud (default 5M points, gs_train.synthetic.
     street_cloud over a 1M-point truth street), wall clock per build after a warm-up, and the bytes
     the index holds
  2. the chunk loop's densify events (TrainChunk.events[...]["ms_densify"]) on one synthetic street
     chunk and seed, with and without the cloud: two chunks advanced in lock step, so their events
     alternate in time; the first event of each is the warm-up and is left out of the medians.
     ms_densify is the host clock over the densify call (it waits for the plan's counts; the apply
     launch is not waited for), ms the whole event up to a device synchronise
  3. the plan alone on the same rows: gsr_densify_plan against gsr_densify_plan_gt and the query
     kernel alone (gsr_gt_far_mask over every row), device events, interleaved

    python tools/gt_cloud_bench.py [--cloud 5000000] [--rows 970000] [--size 512] [--events 8]

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

import torch  # noqa: E402


def med(v):
    return round(statistics.median(v), 3) if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cloud", type=int, default=5_000_000)
    ap.add_argument("--rows", type=int, default=970_000, help="LiDAR-like initial rows (P = rows + 30k fixed)")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--positions", type=int, default=12)
    ap.add_argument("--events", type=int, default=8)
    ap.add_argument("--interval", type=int, default=10)
    ap.add_argument("--thr", type=float, default=0.05)
    ap.add_argument("--builds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--grad-threshold", type=float, default=0.0008, help="densify_grad_threshold (the tests' scaled "
                    "schedule: a few iterations of statistics already clone and split)")
    ap.add_argument("--percent-dense", type=float, default=0.01)
    ap.add_argument("--one-event", action="store_true", help="one constrained event only (for a kernel trace)")
    a = ap.parse_args()
    from gs_train._native import lib, ptr, stream
    from gs_train.chunk import ChunkSchedule, TrainChunk, street_chunk
    from gs_train.gtcloud import GtPointCloud
    from gs_train.native_step import NativeTrainStep
    dev = torch.device("cuda")
    n_it = a.interval * (a.events + 2)
    sched = lambda: ChunkSchedule(iterations=n_it, densification_interval=a.interval, opacity_reset_interval=10 * n_it,
                                  densify_from_iter=a.interval, densify_until_iter=n_it, sh_interval=1000,
                                  densify_grad_threshold=a.grad_threshold, percent_dense=a.percent_dense)
    kw = dict(W=a.size, H=a.size, positions=a.positions, n_init=a.rows, iterations=n_it, device=dev)
    torch.manual_seed(0)
    ts_gt, info = street_chunk(NativeTrainStep, gt_cloud_points=a.cloud, gt_threshold=a.thr, **kw)
    cloud = info["gt_cloud"]
    out = {"cloud_points": cloud.G, "threshold": a.thr, "cells": cloud.cells, "grid": cloud.grid,
           "index_bytes": cloud.bytes, "bytes_per_point": round(cloud.bytes / cloud.G, 2), "P_init": info["P_init"]}

    # 1. index build
    if not a.one_event:
        pts = torch.tensor(info["gt_points"], device=dev)
        times = []
        for k in range(a.builds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = GtPointCloud(pts, threshold=a.thr)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
            c.close()
        out["build_ms"] = [round(t, 2) for t in times[1:]]
        out["build_ms_median"] = med(times[1:])
        del pts

    # 3. the plan alone, on the chunk's initial rows with statistics that split / clone some
    if not a.one_event:
        g = ts_gt.g
        L = lib()
        P = g.P
        gen = torch.Generator(device=dev).manual_seed(1)
        acc = torch.rand(P, generator=gen, device=dev) * 0.03
        maxr = torch.rand(P, generator=gen, device=dev) * 20
        scratch = torch.empty(L.gsr_densify_scratch_bytes(P), dtype=torch.uint8, device=dev)
        counts = torch.zeros(6, dtype=torch.int64, device=dev)
        mask = torch.empty(P, dtype=torch.uint8, device=dev)
        s = stream(dev)
        common = (P, ts_gt.scaffold, ptr(acc), ptr(maxr), ptr(g._opacity.detach()), ptr(g._scaling.detach()))
        calls = {
            "plan": lambda: L.gsr_densify_plan(*common, 0.015, 0.005, 0.0001 * ts_gt.extent, ptr(scratch), ptr(counts), s),
            "plan_gt": lambda: L.gsr_densify_plan_gt(*common, ptr(g._xyz.detach()), 0.015, 0.005, 0.0001 * ts_gt.extent,
                                                     cloud.handle, a.thr, ptr(scratch), ptr(counts), s),
            "far_mask": lambda: L.gsr_gt_far_mask(P, ptr(g._xyz.detach()), cloud.handle, a.thr, None, ptr(mask), s),
        }
        ms = {k: [] for k in calls}
        for rep in range(a.reps + 3):
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                assert fn() == 0
                e1.record()
                e1.synchronize()
                if rep >= 3:
                    ms[k].append(e0.elapsed_time(e1))
        out["plan_rows"] = P
        out["plan_counts_gt"] = [int(v) for v in counts.cpu()]
        out["plan_ms"] = {k: {"median": med(v), "min": round(min(v), 3)} for k, v in ms.items()}
        out["far_rows_share"] = round(float(mask.float().mean()), 4)

    # 2. the chunk loop's events, the two chunks in lock step
    tc_gt = TrainChunk(ts_gt, sched())
    if a.one_event:
        while not tc_gt.events:
            tc_gt.iteration()
        torch.cuda.synchronize()
        out["event"] = tc_gt.events[0]
        print(json.dumps(out))
        return
    torch.manual_seed(0)
    ts_plain, _ = street_chunk(NativeTrainStep, **kw)
    tc_plain = TrainChunk(ts_plain, sched())
    for it in range(1, n_it):
        for tc in ((tc_plain, tc_gt) if it % 2 else (tc_gt, tc_plain)):
            tc.iteration()
    torch.cuda.synchronize()
    keys = ("iteration", "P_before", "P_after", "ms_densify", "ms", "kept", "cloned", "split", "gt_pruned", "gt_pruned_fixed")
    for name, tc in (("plain", tc_plain), ("gt", tc_gt)):
        ev = [{k: e[k] for k in keys if k in e} for e in tc.events if "total" in e]
        out["events_" + name] = ev
        for f in ("ms_densify", "ms"):  # ms: the whole event, to the device synchronise after it
            out[f + "_" + name] = {"median": med([e[f] for e in ev[1:]]), "min": min(e[f] for e in ev[1:])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
