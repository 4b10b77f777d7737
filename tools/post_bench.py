"""The post-optimisation iteration, Python-driven against native, on bench.py's train_post leg's own
problem (synthetic_post_problem at --post-leaves' default, chunk_size^2, seed 1, 10k skybox rows, 10k
anchors, four views):

  * PostTrainStep and NativePostStep in one process, pre-warmed, alternating for --rounds rounds of
    --steps iterations each (both see the same limit draws: the host generator is re-seeded per
    round); ms per iteration between synchronisations: median and p10-p90 over the rounds;
  * the share of rows live (nonzero moments) after 100, 1000 and 5000 native iterations, with the
    share never reached by any cut (a mark below the iterations the pre-warm and the rounds have already
    run is read at that count: 490 with the defaults);
  * gsr_post_adam_step alone against the three things it replaces (the five zero fills,
    gsr_zero_grad_rows, the dense gsr_sparse_adam_step) on the state at those iteration counts, by
    device events, with the bytes each moves and TB/s.

    python tools/post_bench.py --out profiles/r27_post_bench.txt

Needs the GPU (no fallback).  A smaller --leaves / --size is a rehearsal of the script, not a
measurement."""
from __future__ import annotations

import argparse
import ctypes
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "street-sparse-3dgs_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

WIDTHS = (3, 48, 1, 3, 4)
ROW_FLOATS = sum(WIDTHS)


def pct(xs, q):
    return float(np.percentile(np.asarray(xs, np.float64), q))


def timed_steps(post, steps, seed):
    import torch
    torch.manual_seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        post.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def event_ms(fn, reps, warm=3):
    import torch
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def kernel_alone(native, reps, say):
    """gsr_post_adam_step against what it replaces, on copies of the native step's state."""
    import torch
    import post_adam_cases as C
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    m = native.m
    dev = m._xyz.device
    N, S = m.N, m.skybox_points
    live, stamp, cur = native.row_state()
    params = [m._xyz, m._features, m._opacity, m._scaling, m._rotation]
    P = [p.detach().clone().reshape(N, -1) for p in params]
    M = [native.optimizer.state[p]["exp_avg"].clone().reshape(N, -1) for p in params]
    V = [native.optimizer.state[p]["exp_avg_sq"].clone().reshape(N, -1) for p in params]
    G = [torch.zeros_like(p) for p in P]
    lock = native._lock
    touched = stamp == cur
    locked = torch.zeros(N, dtype=torch.bool, device=dev)
    locked[N - S:] = True
    if lock is not None:
        locked |= lock != 0
    n_step = int((touched & ~locked).sum())
    n_zero = int((touched & locked).sum())
    n_idle = int((~touched & (live != 0)).sum())
    n_none = N - n_step - n_zero - n_idle
    s = C._stream(dev)
    groups = C.make_groups(P, G, M, V, 7)
    ptrs = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in G])
    widths = (ctypes.c_int64 * 5)(*WIDTHS)
    anchors = m.anchors

    def fills():
        for g in G:
            g.zero_()

    def zero_rows():
        C._check(L.gsr_zero_grad_rows(5, ptrs, widths, N, S, anchors.data_ptr() if anchors.numel() else None,
                                      anchors.numel(), s), "gsr_zero_grad_rows")

    def dense():
        C._check(L.gsr_sparse_adam_step(len(groups), groups, N, None, 0.9, 0.999, 1e-15, None, s), "dense Adam")

    def post():
        C._check(L.gsr_post_adam_step(len(groups), groups, N, stamp.data_ptr(), cur, live.data_ptr(), S,
                                      lock.data_ptr() if lock is not None else None, 0.9, 0.999, 1e-15, s), "post Adam")

    t_fill, t_zero, t_dense, t_post = (event_ms(f, reps) for f in (fills, zero_rows, dense, post))
    f4 = 4 * ROW_FLOATS
    b_fill = N * f4
    b_zero = (S + anchors.numel()) * f4
    b_dense = 7 * N * f4                      # g, p, m, v read; p, m, v written
    b_post = (8 * n_step + 6 * n_idle + n_zero) * f4 + 5 * 6 * N   # + the row state per array
    tb = lambda b, ms: b / (ms * 1e-3) / 1e12
    say(f"    rows {N}: stamped+unlocked {n_step} ({n_step / N:.1%}), stamped+locked {n_zero}, idle live {n_idle} "
        f"({n_idle / N:.1%}), untouched {n_none} ({n_none / N:.1%})")
    say(f"    five zero fills        {t_fill:8.4f} ms  {b_fill / 1e6:9.1f} MB  {tb(b_fill, t_fill):5.2f} TB/s")
    say(f"    gsr_zero_grad_rows     {t_zero:8.4f} ms  {b_zero / 1e6:9.1f} MB")
    say(f"    dense sparse_adam_step {t_dense:8.4f} ms  {b_dense / 1e6:9.1f} MB  {tb(b_dense, t_dense):5.2f} TB/s")
    say(f"    the three together     {t_fill + t_zero + t_dense:8.4f} ms")
    say(f"    gsr_post_adam_step     {t_post:8.4f} ms  {b_post / 1e6:9.1f} MB  {tb(b_post, t_post):5.2f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=3_000_000, help="bench.py --post-leaves' default")
    ap.add_argument("--size", type=int, default=1536, help="bench.py --chunk-size's default")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--steps", type=int, default=40, help="iterations per round and class")
    ap.add_argument("--marks", default="100,1000,5000", help="native iteration counts at which the live share is read")
    ap.add_argument("--reps", type=int, default=20, help="repetitions of each call of the kernel-alone part")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("post_bench.py needs a ROCm GPU")
    from gs_train.native_post import NativePostStep
    from gs_train.post import PostTrainStep, synthetic_post_problem
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    W = H = a.size
    steps = {}
    for cls in (PostTrainStep, NativePostStep):
        torch.manual_seed(0)
        steps[cls] = synthetic_post_problem(a.leaves, W, H, n_views=4, skybox=10_000, n_anchors=10_000, seed=1,
                                            step_cls=cls)
    py, nat = steps[PostTrainStep], steps[NativePostStep]
    say(f"post_bench: {a.leaves} leaves, {py.m.N} rows, {W}x{H}, 4 views, 10k skybox rows, 10k anchors; "
        f"{torch.cuda.get_device_name(0)}")
    for post in (py, nat):  # pre-warm both on the same draws
        timed_steps(post, 10, seed=123)
    t_py, t_nat = [], []
    for r in range(a.rounds):
        t_py.append(timed_steps(py, a.steps, seed=1000 + r))
        t_nat.append(timed_steps(nat, a.steps, seed=1000 + r))
    say(f"ms per iteration, {a.rounds} alternating rounds of {a.steps} iterations (host clock between synchronisations):")
    for name, t in (("PostTrainStep ", t_py), ("NativePostStep", t_nat)):
        say(f"  {name} median {pct(t, 50):.4f}  p10 {pct(t, 10):.4f}  p90 {pct(t, 90):.4f}  min {min(t):.4f}  max {max(t):.4f}")
    say(f"  native median / python median = {pct(t_nat, 50) / pct(t_py, 50):.4f}; native median "
        f"{'below' if pct(t_nat, 50) < pct(t_py, 10) else 'NOT below'} the python p10")
    say("live rows (nonzero moments) and rows no cut has reached, by native iterations done:")
    for mark in sorted(int(x) for x in a.marks.split(",") if x):
        torch.manual_seed(77)
        while nat.iteration - 1 < mark:
            nat.step()
        live, stamp, _ = nat.row_state()
        N = live.numel()
        say(f"  after {nat.iteration - 1} iterations: live {int((live != 0).sum())} of {N} "
            f"({float((live != 0).float().mean()):.2%}); never stamped by this context {float((stamp == 0).float().mean()):.2%}")
        kernel_alone(nat, a.reps, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
