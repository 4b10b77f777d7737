"""Cases of gsr_post_adam_step (include/gsr_post.h) against the path it replaces: zero-filled
gradients with the touched rows' values written in, gsr_zero_grad_rows, then the dense
gsr_sparse_adam_step -- over the post-optimisation's five arrays (3, 48 with the DC / rest column
split, 1, 3, 4 floats per row).

Row counts: 1, 2; 42 / 43 / 44 (the flat kernel's first 2048-float block ends inside SH row 42);
682 / 683 (the same for the 3-float arrays); 4099 (several workgroups, a ragged last 64-row tile);
70 001.  For each, every touched set meets every tail, with the anchor sets and the moment kinds
rotated through them (combos)."""
from __future__ import annotations

import ctypes

import torch

ROWS = (1, 2, 42, 43, 44, 682, 683, 4099, 70_001)
WIDTHS = (3, 48, 1, 3, 4)           # xyz, features (16 x 3), opacity, scaling, rotation
SPLITS = {1: ((0, 3), (3, 48))}     # the SH buffer is two groups: DC and rest columns
TOUCHED = ("empty", "all", "alternate", "first", "last")
ANCHORS = ("none", "repeats", "touched", "all")
MOMENTS = ("zero", "special")
BETAS, EPS = (0.9, 0.999), 1e-15


def tails(N):
    return (0, min(5, N), N)


def combos(N):
    """(touched, tail, anchors, moments): touched x tail in full, the other two rotated."""
    out = []
    for i, t in enumerate(TOUCHED):
        for j, tail in enumerate(tails(N)):
            out.append((t, tail, ANCHORS[(i + j) % 4], MOMENTS[(i + j) % 2]))
    return out


def touched_rows(kind, N, dev):
    if kind == "empty":
        return torch.empty(0, dtype=torch.int64, device=dev)
    if kind == "all":
        return torch.arange(N, device=dev)
    if kind == "alternate":
        return torch.arange(0, N, 2, device=dev)
    return torch.tensor([0 if kind == "first" else N - 1], device=dev)


def anchor_rows(kind, N, touched, g, dev):
    if kind == "none":
        return torch.empty(0, dtype=torch.int64, device=dev)
    if kind == "all":
        return torch.arange(N, device=dev)
    if kind == "repeats":
        a = torch.randint(0, N, (max(2, N // 7),), generator=g, device=dev)
        return torch.cat([a, a[:1], a[:1]])
    # one anchor that is also touched (when any row is), one that is not necessarily
    extra = torch.randint(0, N, (1,), generator=g, device=dev)
    return torch.cat([touched[:1], extra]) if touched.numel() else extra


SPECIALS = (0.0, -0.0, float("nan"), float("inf"), -float("inf"))


def make_state(N, moments, touched, g, dev):
    """Parameters (with a -0.0 and a +0.0 among them), moments and the dense gradients (zero, the
    touched rows' values written in: random, and +-0 / NaN / +-Inf in the first touched rows)."""
    P = [torch.randn(N, w, generator=g, device=dev) for w in WIDTHS]
    P[0][0, 0] = -0.0
    P[2][N - 1, 0] = 0.0
    M = [torch.zeros(N, w, device=dev) for w in WIDTHS]
    V = [torch.zeros(N, w, device=dev) for w in WIDTHS]
    if moments == "special":
        idle = torch.ones(N, dtype=torch.bool, device=dev)
        idle[touched] = False
        rows = idle.nonzero().flatten()
        # untouched rows: trained-looking moments in some, a lone -0.0 in one, a lone denormal in another
        for k, r in enumerate(rows[:: max(1, rows.numel() // 40)].tolist()):
            if k % 3 == 0:
                for m_, v_ in zip(M, V):
                    m_[r] = 0.01 * torch.randn(m_.shape[1], generator=g, device=dev)
                    v_[r] = 1e-4 * torch.rand(v_.shape[1], generator=g, device=dev)
            elif k % 3 == 1:
                M[1][r, 47] = -0.0
            else:
                V[4][r, 3] = 1e-45
        # and moments in the touched rows too (a row trained before)
        for m_, v_ in zip(M, V):
            m_[touched[::3]] = 0.01 * torch.randn(touched[::3].numel(), m_.shape[1], generator=g, device=dev)
            v_[touched[::3]] = 1e-4 * torch.rand(touched[::3].numel(), v_.shape[1], generator=g, device=dev)
    G = [torch.zeros(N, w, device=dev) for w in WIDTHS]
    for gk in G:
        gk[touched] = torch.randn(touched.numel(), gk.shape[1], generator=g, device=dev)
    for j, r in enumerate(touched[:10].tolist()):
        for gk in G:
            gk[r, j % gk.shape[1]] = SPECIALS[j % len(SPECIALS)]
    return P, M, V, G


def make_groups(P, G, M, V, step):
    """The six gsr_adam_groups (xyz, f_dc, f_rest, opacity, scaling, rotation) with the bias
    corrections of Adam step `step` and train_post's learning rates."""
    import math
    from diff_gaussian_rasterization._lib import AdamGroup
    lrs = {0: (1.6e-4,), 1: (5e-4, 5e-4 / 20), 2: (0.01,), 3: (1e-3,), 4: (1e-3,)}
    b1, b2 = BETAS
    out = []
    for k, w in enumerate(WIDTHS):
        for (c0, c1), lr in zip(SPLITS.get(k, ((0, w),)), lrs[k]):
            off = 4 * c0
            out.append(AdamGroup(P[k].data_ptr() + off, G[k].data_ptr() + off, M[k].data_ptr() + off,
                                 V[k].data_ptr() + off, c1 - c0, lr / (1 - b1 ** step), math.sqrt(1 - b2 ** step), w))
    return (AdamGroup * len(out))(*out)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check(rc, what):
    from diff_gaussian_rasterization import _lib
    assert rc == 0, (what, rc, _lib.last_error())


def reference_step(P, G, M, V, tail, anchors, step):
    """The path the kernel replaces, in place on P, M, V, G: gsr_zero_grad_rows, then the dense step."""
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    N, dev = P[0].shape[0], P[0].device
    ptrs = (ctypes.c_void_p * len(G))(*[t.data_ptr() for t in G])
    widths = (ctypes.c_int64 * len(G))(*WIDTHS)
    _check(L.gsr_zero_grad_rows(len(G), ptrs, widths, N, tail, anchors.data_ptr() if anchors.numel() else None,
                                anchors.numel(), _stream(dev)), "gsr_zero_grad_rows")
    groups = make_groups(P, G, M, V, step)
    _check(L.gsr_sparse_adam_step(len(groups), groups, N, None, BETAS[0], BETAS[1], EPS, None, _stream(dev)),
           "gsr_sparse_adam_step")


def live_build(M, V, dev):
    from diff_gaussian_rasterization import _lib
    N = M[0].shape[0]
    live = torch.full((N,), 7, dtype=torch.uint8, device=dev)
    groups = make_groups(M, M, M, V, 1)  # only the moment pointers are read
    _check(_lib.load().gsr_post_live_build(len(groups), groups, N, live.data_ptr(), _stream(dev)), "gsr_post_live_build")
    return live


def post_step(P, G, M, V, stamp, cur, live, tail, lock, step):
    from diff_gaussian_rasterization import _lib
    N, dev = P[0].shape[0], P[0].device
    groups = make_groups(P, G, M, V, step)
    _check(_lib.load().gsr_post_adam_step(len(groups), groups, N, stamp.data_ptr(), cur, live.data_ptr(), tail,
                                          lock.data_ptr() if lock is not None else None, BETAS[0], BETAS[1], EPS,
                                          _stream(dev)), "gsr_post_adam_step")


def bits(t):
    return t.contiguous().view(torch.int32)
