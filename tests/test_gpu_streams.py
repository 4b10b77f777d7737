"""Atomic-mode backwards handed between streams and host threads.

The backward's accumulator rows are one grow-only array per device (rasterizer.hip AccRows), leased
to one backward at a time: a backward on another stream than the previous one first waits for the
device, and a larger frame grows the array in stream order.  Two scenes alternate between the
default stream and a second stream -- driven by the same host thread, and by a second host thread
(whose first forward has no capacity hint and reads K before the binning; torch runs every backward
on its autograd thread) -- and each run must reproduce its scene's reference.
"""
from __future__ import annotations

import threading

import pytest

from helpers import settings, torch_inputs
from test_gpu_parity import make_scene, upstream_grads

# B has more rows than A: the device's row array grows when B follows A
A = dict(name="streams_a", P=2000, W=96, H=64, deg=3, seed=41, log_scale=-3.2)
B = dict(name="streams_b", P=6000, W=128, H=96, deg=3, seed=42, log_scale=-3.2)
# two atomic-mode backwards of one frame (test_backward_twice_through_saved_buffers)
ATOMIC_TOL = 1e-5


def fwd_bwd(c):
    """One forward + backward of scene c on the current stream: (color, radii, invdepth, gradients)."""
    import torch
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = torch.device("cuda:0")
    s = make_scene(c)
    dcol, dinv = upstream_grads(c)
    inp = torch_inputs(s, dev)
    color, radii, invd = GaussianRasterizer(settings(s, dev, 3))(**inp)
    ((color * torch.tensor(dcol, device=dev)).sum() + (invd * torch.tensor(dinv, device=dev)).sum()).backward()
    return color.detach(), radii, invd.detach(), [v.grad for v in inp.values()]


def check(got, ref, what):
    import torch
    assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2]), f"{what}: image differs from the reference"
    assert torch.equal(got[1], ref[1]), f"{what}: radii differ from the reference"
    for k, (g, r) in enumerate(zip(got[3], ref[3])):
        e = float((g - r).norm() / max(float(r.norm()), 1e-30))
        print(f"{what}: gradient {k} rel L2 {e:.3e}")
        assert e < ATOMIC_TOL, f"{what}: gradient {k} rel L2 {e}"
    assert any(float(r.norm()) > 0 for r in ref[3])


def hand_over(run_on_second):
    """Reference of A and B on the default stream; then A (default), B (second), A, B again."""
    import torch
    from diff_gaussian_rasterization import _C
    prev = _C.set_deterministic(False)
    try:
        ref_a, ref_b = fwd_bwd(A), fwd_bwd(B)
        a1 = fwd_bwd(A)
        b1 = run_on_second(B)
        a2 = fwd_bwd(A)
        b2 = run_on_second(B)
        torch.cuda.synchronize()
    finally:
        _C.set_deterministic(prev)
    check(a1, ref_a, "A, first")
    check(b1, ref_b, "B, first")
    check(a2, ref_a, "A, second")
    check(b2, ref_b, "B, second")


@pytest.mark.gpu
def test_backward_alternates_between_two_streams():
    import torch
    s2 = torch.cuda.Stream()

    def on_s2(c):
        with torch.cuda.stream(s2):
            return fwd_bwd(c)

    hand_over(on_s2)


@pytest.mark.gpu
def test_backward_alternates_between_two_host_threads():
    """The second stream's steps run in a host thread of their own (started and joined before the
    next step: the hand-over is sequential), each thread with its own stream."""
    import torch

    def in_thread(c):
        out = {}

        def body():
            try:
                with torch.cuda.stream(torch.cuda.Stream()):
                    out["r"] = fwd_bwd(c)
            except BaseException as e:  # re-raised in the test's thread
                out["e"] = e

        t = threading.Thread(target=body)
        t.start()
        t.join()
        if "e" in out:
            raise out["e"]
        return out["r"]

    hand_over(in_thread)
