"""Cost of fitting depth maps to the sparse points on one GPU, against the reference's
arithmetic on this host.

A synthetic calibration: `--images` cameras with small random rotations, `--points` sparse points in front
of them (ids a random permutation with gaps), `--obs` observations per image (10% of them -1, as COLMAP's
unmatched keypoints; positions uniform over a 2 size x 2 size image, s = 1/2), one size x size 16-bit map
of noise per image, generated on the device.

  1. the fit kernel alone: gsr_depth_scale_fit on prepared device arrays, device events, median of --reps
     after a warm-up; its launches counted (one, whatever the batch) with the bytes the rule needs
  2. the whole call gs_train.depth_scale.fit_depth_scales, inputs on the device: wall clock around a call
     that ends in its copy of the records (the id table's two synchronising entry points included)
  3. `literal` of tests/depth_scale_ref.py (the reference line by line, numpy's median and mean) over the
     first --cpu-images images in a pool of --threads threads, wall clock, scaled to --images; its scale
     and offset are compared with the device's on those images

    python tools/depth_scale_bench.py [--images 1500] [--obs 4000] [--size 1536] [--points 2000000]
                                      [--cpu-images 96 (0: skip 3)] [--threads 16] [--out profiles/r24_depth_scale_bench.txt]
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import ctypes
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "street-sparse-3dgs_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def synthetic(images, obs, size, points, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    rng = np.random.default_rng(seed)
    ax = rng.normal(size=(images, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = rng.uniform(0, 0.3, images)
    q = np.concatenate([np.cos(ang / 2)[:, None], np.sin(ang / 2)[:, None] * ax], 1)
    t = rng.normal(size=(images, 3)) * 0.5
    sizes = np.full((images, 2), 2 * size, np.int64)
    xyz = torch.rand((points, 3), generator=g, device=dev, dtype=torch.float64) * torch.tensor(
        [40.0, 40.0, 78.0], device=dev, dtype=torch.float64) + torch.tensor([-20.0, -20.0, 2.0], device=dev,
                                                                             dtype=torch.float64)
    ids = (torch.randperm(points, generator=g, device=dev) * 5) // 4  # unique, with gaps
    O = images * obs
    pid = ids[torch.randint(0, points, (O,), generator=g, device=dev)]
    pid[torch.rand(O, generator=g, device=dev) < 0.1] = -1
    xy = torch.rand((O, 2), generator=g, device=dev, dtype=torch.float64) * (2 * size)
    ptr = np.arange(images + 1, dtype=np.int64) * obs
    maps = torch.empty((images, size, size), dtype=torch.int16, device=dev)
    for k0 in range(0, images, 64):
        n = min(64, images - k0)
        maps[k0:k0 + n] = torch.randint(-32768, 32768, (n, size, size), generator=g, device=dev, dtype=torch.int16)
    return q, t, sizes, ptr, xy, pid, ids, xyz, maps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1500)
    ap.add_argument("--obs", type=int, default=4000)
    ap.add_argument("--size", type=int, default=1536)
    ap.add_argument("--points", type=int, default=2000000)
    ap.add_argument("--cpu-images", type=int, default=96)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_scale_bench: needs a ROCm GPU")
    from gs_train import depth_scale as D
    from gs_train._native import check, lib, ptr, stream
    dev = torch.device("cuda")
    q, t, sizes, ptr_h, xy, pid, ids, xyz, maps = synthetic(a.images, a.obs, a.size, a.points, dev)
    M, O, N = a.images, a.images * a.obs, a.points
    lines = [f"depth_scale_bench: {M} images x {a.obs} observations, maps {a.size}^2, {N} points, torch "
             f"{torch.__version__}, {torch.cuda.get_device_name(0)}"]

    # 1. the kernel alone
    L = lib()
    mm = (ctypes.c_int64 * 2)()
    s = stream(dev)
    check(L.gsr_chunk_id_range(N, ptr(ids), mm, s), "gsr_chunk_id_range")
    T = int(mm[1]) + 1
    table = torch.empty(T, dtype=torch.int32, device=dev)
    check(L.gsr_chunk_id_table(N, ptr(ids), T, ptr(table), s), "gsr_chunk_id_table")
    cams = torch.from_numpy(D.camera_table(q, t, sizes, np.arange(M))).to(dev)
    off = torch.from_numpy(ptr_h).to(dev)
    scratch = torch.empty(int(L.gsr_depth_scale_scratch_bytes(O)), dtype=torch.uint8, device=dev)
    rec = torch.zeros(M * D.RECORD.itemsize, dtype=torch.uint8, device=dev)

    def kernel():
        check(L.gsr_depth_scale_fit(M, ptr(cams), ptr(off), O, None, O, ptr(xy), ptr(pid), N, T, ptr(table), ptr(xyz), M,
                                    a.size, a.size, ptr(maps), 0, ptr(scratch), ptr(rec), s), "gsr_depth_scale_fit")

    for _ in range(3):
        kernel()
    torch.cuda.synchronize()
    first = rec.cpu().numpy().copy()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        kernel()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    assert np.array_equal(rec.cpu().numpy(), first), "two runs differ"
    r = first.view(D.RECORD)
    k_ms = statistics.median(times)
    # per observation: id 8 B + position 16 B; per masked one a table entry 4 B and a point 24 B; per valid one
    # four 2-B samples, each its own 64-B line in a map of noise
    masked = int((pid >= 0).sum())
    valid = int(r["n_valid"].sum())
    need = 24 * O + 28 * masked + 8 * valid
    lines.append(f"fit kernel: {k_ms * 1e3:.0f} us (median of {a.reps}, device events; min {min(times) * 1e3:.0f}, max "
                 f"{max(times) * 1e3:.0f}), 1 launch of {M} workgroups for the batch, no host read; {valid} valid of {O} "
                 f"observations, {int((r['flags'] & 1).sum())} images fitted; {need / 1e6:.0f} MB needed = "
                 f"{need / k_ms / 1e9:.2f} TB/s of algorithmic bytes ({valid * 4 * 64 / 1e6:.0f} MB of 64-B lines behind "
                 f"the map samples)")

    # 2. the whole call
    kw = dict(qvecs=q, tvecs=t, sizes=sizes, obs_ptr=ptr_h, obs_xy=xy, obs_point_id=pid, point_id=ids, point_xyz=xyz,
              maps=maps)
    fit = D.fit_depth_scales(**kw)
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit = D.fit_depth_scales(**kw)
        walls.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(fit.scale, r["scale"], equal_nan=True)
    lines.append(f"fit_depth_scales, inputs on the device: {statistics.median(walls):.2f} ms wall clock (median of 5; the "
                 f"camera table made on the host, the id table over {N} points and the copy of the records included)")

    # 3. the reference's arithmetic on this host
    import depth_scale_ref as R
    K = min(a.cpu_images, M)
    if K < 1:
        print("\n".join(lines))
        return
    xy_h, pid_h = xy[:K * a.obs].cpu().numpy(), pid[:K * a.obs].cpu().numpy()
    ids_h, xyz_h = ids.cpu().numpy(), xyz.cpu().numpy()
    maps_h = maps[:K].cpu().numpy().view(np.uint16)
    ordered = np.zeros([ids_h.max() + 1, 3])
    ordered[ids_h] = xyz_h

    def one(k):
        return R.literal(q[k], t[k], int(sizes[k, 0]), int(sizes[k, 1]), xy_h[k * a.obs:(k + 1) * a.obs],
                         pid_h[k * a.obs:(k + 1) * a.obs], ids_h, xyz_h, maps_h[k], ordered=ordered)

    one(0)
    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(max_workers=a.threads) as ex:
        got = list(ex.map(one, range(K)))
    cpu_s = time.perf_counter() - t0
    worst = 0.0
    for k, g in enumerate(got):
        assert g["n_valid"] == int(r["n_valid"][k])
        if g["scale"]:
            worst = max(worst, abs(g["scale"] - r["scale"][k]) / abs(g["scale"]),
                        abs(g["offset"] - r["offset"][k]) / (abs(g["t_colmap"]) + abs(g["t_mono"] * g["scale"])))
    lines.append(f"literal (numpy, the sample restated, the zero-row point table built once) on {K} images, {a.threads} "
                 f"threads: {cpu_s * 1e3:.0f} ms = {cpu_s / K * 1e3:.2f} ms per image, {cpu_s / K * M:.2f} s for {M} "
                 f"images at that rate; the kernel is {cpu_s / K * M / (k_ms * 1e-3):.0f}x, the whole call "
                 f"{cpu_s / K * M / (statistics.median(walls) * 1e-3):.0f}x; largest relative distance of scale / offset "
                 f"on those images {worst:.2e} (numpy's float32 mean of s_mono)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
