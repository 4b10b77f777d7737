"""Measurements of the training-view stage (csrc/views.hip, gs_train/views.py) on the GPU:

  1. gsr_view_expand at size x size with every plane (RGB8 + mask8 + depth16 in, six float32 planes out):
     device-event time per launch, once on one view (its 71 MB stay in the 256 MiB Infinity Cache) and
     once rotating over enough views and plane sets to exceed it; bytes moved over time against the
     HBM peak (8.0 TB/s spec, 6.29 TB/s measured float4 copy);
  2. the Lanczos resize of a (2 size)^2 RGB image to size^2 (both passes, 13 taps each);
  3. the native train step on harness.make_problem's scene at size x size (4 views, 90 degree faces,
     alpha masks, depth, skybox rows), fed by plain lists and by a ViewStore with 2 plane sets, in
     interleaved blocks: median and spread of each feed;
  4. the memory table for 192 and 2000 views from ViewStore.nbytes().

    python tools/views_bench.py [--size 1536] [--out profiles/r22_views_bench.txt]

There is no CPU path: without a GPU the script fails."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "street-sparse-3dgs_amd")]

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12  # bytes / s: the spec peak and the measured float4 copy rate


def event_ms(fn, iters, warmup=5):
    import torch
    for _ in range(warmup):
        fn(0)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel_us(fn, iters=24):
    """Median device time of one call's launches, in microseconds: the stream is first kept busy with
    fills so that the host runs ahead and each event pair brackets the kernel alone, not the Python
    call that enqueues it."""
    import torch
    filler = torch.empty(1 << 31, dtype=torch.uint8, device="cuda")
    for i in range(4):
        fn(i)
    torch.cuda.synchronize()
    for _ in range(12):
        filler.fill_(1)
    pairs = []
    for i in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in pairs) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1536)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r22_views_bench.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("views_bench: needs a ROCm GPU")
    from gs_train.harness import make_problem
    from gs_train.native_step import NativeTrainStep
    from gs_train.synthetic import orbit_cameras
    from gs_train.views import ResizePlan, ViewStore
    dev = "cuda"
    S = a.size
    lines = [f"views_bench: size {S} x {S}, torch {torch.__version__}, {torch.cuda.get_device_name(0)}"]
    say = lambda s: (lines.append(s), print(s, flush=True))
    g = torch.Generator().manual_seed(1)

    # 1. the expansion
    n_views, n_sets = 8, 4
    store = ViewStore(dev, slots=n_sets)
    for _ in range(n_views):
        store.add(image=torch.randint(0, 256, (S, S, 3), generator=g, dtype=torch.uint8),
                  mask=torch.randint(0, 256, (S, S), generator=g, dtype=torch.uint8),
                  invdepth_u16=torch.randint(0, 65536, (S, S), generator=g, dtype=torch.int32), scale=0.7, offset=-0.05)
    nb = store.nbytes()
    b_in, b_out = nb["compact"] // n_views, nb["expanded"] // n_views
    one = ViewStore(dev, slots=1)  # slots=1: every touch of another view expands; two views alternate in cache
    one._views = store._views[:2]
    hot, cold = (lambda i: one.gts[i & 1]), (lambda i: store.gts[i % n_views])
    for tag, fn, ws in (("2 views, 1 plane set", hot, 2 * b_in + b_out),
                        (f"{n_views} views, {n_sets} plane sets", cold, n_views * b_in + n_sets * b_out)):
        us, loop_us = kernel_us(fn), event_ms(fn, 200) * 1e3
        rate = (b_in + b_out) / (us * 1e-6)
        say(f"expand {tag} (working set {ws / 1e6:.0f} MB): kernel {us:.1f} us (median of 24, device events), "
            f"{b_in / 1e6:.1f} MB in + {b_out / 1e6:.1f} MB out = {rate / 1e12:.2f} TB/s, "
            f"{100 * rate / HBM_SPEC:.0f}% of the 8.0 TB/s spec, {100 * rate / HBM_COPY:.0f}% of the measured copy rate; "
            f"{loop_us:.1f} us per view in a back-to-back loop of store.gts[k] (the Python call included)")

    # 2. the resize
    big = torch.randint(0, 256, (2 * S, 2 * S, 3), generator=g, dtype=torch.uint8).to(dev)
    plan = ResizePlan(2 * S, 2 * S, S, S)
    ms_rs = event_ms(lambda i: plan.resize(big), 50)
    info = plan.info()
    say(f"resize {2 * S}^2 -> {S}^2 RGB: {ms_rs * 1e3:.0f} us per image (back-to-back loop, both passes, {info['ksize_x']} and "
        f"{info['ksize_y']} taps, tables {info['table_bytes']} B, uploads {info['uploads']}); reads "
        f"{big.numel() / 1e6:.1f} MB, writes {(S * 2 * S * 3 + S * S * 3) / 1e6:.1f} MB, rereads {S * 2 * S * 3 / 1e6:.1f} MB")
    del big, store, one
    torch.cuda.empty_cache()

    # 3. the native step fed by lists and by the store
    steps = {}
    for fed in ("lists", "store"):
        torch.manual_seed(0)
        ts = make_problem(a.gaussians, S, S, n_views=4, seed=1, step_cls=NativeTrainStep, alpha=True,
                          skybox_points=10_000, fovx_deg=90.0)
        vs = ViewStore(dev, slots=2)
        for k in range(4):
            d = ts.mono[k][0]
            scale = float(d.max()) * 1.01 + 1e-3
            vs.add(image=torch.round(ts.gts[k].clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).contiguous(),
                   mask=(ts.amask[k][0] * 255).to(torch.uint8),
                   invdepth_u16=torch.clamp(torch.round(d / scale * 65536.0), 0, 65535).to(torch.int32), scale=scale)
        if fed == "lists":  # the same planes, resident as float32
            feed = [[seq[k].clone() for k in range(4)] for seq in (vs.gts, vs.alpha_masks, vs.mono_invdepths, vs.depth_masks)]
        else:
            feed = [vs.gts, vs.alpha_masks, vs.mono_invdepths, vs.depth_masks]
        steps[fed] = NativeTrainStep(ts.g, orbit_cameras(4, S, S, fovx_deg=90.0), feed[0], S, S, mono_invdepths=feed[2],
                                     depth_masks=feed[3], alpha_masks=feed[1], skybox_points=10_000)
        steps[fed + "_store"] = vs
        del ts
    for fed in ("lists", "store"):
        for _ in range(12):
            steps[fed].step()
    torch.cuda.synchronize()
    ms = {"lists": [], "store": []}
    for _ in range(a.blocks):
        for fed in ("lists", "store"):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                steps[fed].step()
            torch.cuda.synchronize()
            ms[fed].append((time.perf_counter() - t0) / a.steps * 1e3)
    for fed in ("lists", "store"):
        v = ms[fed]
        say(f"native step fed by {fed}: median {statistics.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f} "
            f"({a.blocks} interleaved blocks of {a.steps} steps, {a.gaussians} Gaussians, 4 views cycled)")
    say(f"store minus lists: {statistics.median(ms['store']) - statistics.median(ms['lists']):+.3f} ms per step; "
        f"expansions {steps['store_store'].expansions} in the store-fed run")

    # 4. the memory table (the same device tensors added N times: nbytes() counts each view's own bytes)
    v0 = steps["store_store"]._views[0]
    for n in (192, 2000):
        st = ViewStore(dev, slots=2)
        st._views = [v0] * n
        nb = st.nbytes()
        say(f"memory, {n} views of {S}^2 with mask and depth: compact {nb['compact'] / 1e9:.2f} GB + 2 plane sets "
            f"{nb['planes'] / 1e6:.0f} MB; as resident float32 planes {nb['expanded'] / 1e9:.2f} GB "
            f"({nb['expanded'] / (nb['compact'] + nb['planes']):.2f}x)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
