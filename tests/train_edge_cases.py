"""Seeded inputs and fp64 torch references for the image side of a training iteration at ragged
sizes and exact ties: the exposure affine, L1 + SSIM, the masked inverse-depth L1, the depth-only
loss and their composition (csrc/loss.hip).  tests/test_gpu_train_edges.py runs the kernels on
these; tests/test_train_cpu.py checks that the inputs are well conditioned.  Importable without a GPU.

Every builder returns CPU float32 tensors; every reference evaluates those same float32 numbers in
float64 (or, with dtype=torch.float32, in float32 -- the yardstick of the conditioning checks).
"""
from __future__ import annotations

import torch

import train_ref as TR

# ---- exposure ------------------------------------------------------------------------------------
# exposure_blocks() caps the grid at 1024 blocks of 256 threads: 512 x 512 = 262,144 px is the last
# size every thread handles in one trip, 5 x 52429 is one pixel into the second trip, 577 x 911 a
# partly filled third trip.
EXPOSURE_SIZES = [(1, 1), (1, 255), (1, 257), (512, 512), (5, 52429), (577, 911)]
# Each dE entry is an fp32 sum whose tree is at most 40 deep (3 per thread, 6 in the wave, 4 in the
# block, 16 per lane of the finalize, 6 in its wave), so |dE - ref| <= 40 * 2^-24 * sum|terms|
# ~ 2.4e-6 * sum|terms|.
EXPOSURE_DE_BOUND = 4e-6
CLAMP_MARGIN = 1e-5  # no pre-clamp value this close to 0 or 1: fp32 and fp64 clamp alike
TIE_COLOURS = (-0.5, 0.0, 0.25, 1.0, 1.5)


def exposure_pre(color, E):
    """matmul(color.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]."""
    return torch.matmul(color.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]


def _off_the_clamp_edges(color, E):
    """Pixels whose pre-clamp value (fp64) lies within CLAMP_MARGIN of 0 or 1 become mid-grey: there
    an fp32 evaluation may clamp where fp64 does not, which is rounding, not an error."""
    for _ in range(4):
        pre = exposure_pre(color.double(), E.double())
        near = ((pre.abs() < CLAMP_MARGIN) | ((pre - 1).abs() < CLAMP_MARGIN)).any(dim=0)
        if not bool(near.any()):
            return color
        color = torch.where(near[None], torch.full_like(color, 0.5), color)
    raise AssertionError("exposure inputs: a pre-clamp value stays on a clamp edge")


def exposure_inputs(H, W, localised=False):
    """(color, E, upstream): colours in [-0.2, 1.2], E = identity + 0.1 randn, a randn upstream --
    or (localised) one that is zero except on the first 3 and the last 300 pixels of each plane, so
    that sum|terms| is small and one lost or doubled tail pixel stands far above the dE bound."""
    g = torch.Generator().manual_seed(1000 * H + W)
    color = torch.rand(3, H, W, generator=g) * 1.4 - 0.2
    E = torch.eye(3, 4) + 0.1 * torch.randn(3, 4, generator=g)
    up = torch.randn(3, H, W, generator=g)
    if localised:
        keep = torch.zeros(H * W, dtype=torch.bool)
        keep[:3] = True
        keep[-300:] = True
        up = up * keep.view(1, H, W)
    return _off_the_clamp_edges(color, E), E, up


def exposure_tie_inputs(H, W):
    """The exact identity exposure over colours drawn from TIE_COLOURS: every product is exact, so
    pre-clamp values of exactly 0 and exactly 1 occur, where torch.clamp passes the gradient."""
    g = torch.Generator().manual_seed(77 + H * W)
    pick = torch.randint(0, len(TIE_COLOURS), (3, H, W), generator=g)
    color = torch.tensor(TIE_COLOURS)[pick]
    up = torch.randn(3, H, W, generator=g)
    up[up == 0] = 1.0
    return color, torch.eye(3, 4), up


def exposure_terms(color, gmasked):
    """sum|terms| of each dE entry: dE[k][c] = sum_p color_k g_c (c < 3), dE[c][3] = sum_p g_c for the
    clamp-masked upstream g."""
    t = torch.zeros(3, 4, dtype=torch.float64)
    t[:, :3] = torch.einsum("kp,cp->kc", color.double().reshape(3, -1).abs(), gmasked.reshape(3, -1).abs())
    t[:, 3] = gmasked.reshape(3, -1).abs().sum(dim=1)
    return t


def exposure_ref(color, E, up, dtype=torch.float64):
    """out, dL/dcolor, dL/dE for L = sum(out * up), and sum|terms| per dE entry (always fp64)."""
    c = color.detach().clone().to(dtype).requires_grad_(True)
    e = E.detach().clone().to(dtype).requires_grad_(True)
    pre = exposure_pre(c, e)
    out = pre.clamp(0, 1)
    (out * up.to(dtype)).sum().backward()
    passes = ((pre >= 0) & (pre <= 1)).detach()
    return out.detach(), c.grad, e.grad, exposure_terms(color, up.double() * passes)


# ---- L1 + SSIM -----------------------------------------------------------------------------------
SSIM_SHAPES = [(1, 1, 1), (1, 5, 9), (1, 10, 70), (3, 11, 11), (2, 17, 65), (1, 63, 64), (3, 65, 63), (1, 129, 130)]
EDGE_SHAPE = (3, 77, 131)
SSIM_CASES = ["x".join(map(str, s)) for s in SSIM_SHAPES] + ["out_of_range", "ties"]
FLAT_CASES = {"flat_0.7_0.4": (0.7, 0.4), "flat_0.5_0.5": (0.5, 0.5), "flat_1_1": (1.0, 1.0), "flat_0_0": (0.0, 0.0)}
SSIM_UP = (0.8, -0.2)
VALUE_BAR, GRAD_BAR = 2e-6, 1e-5  # tests/test_gpu_train.py: values absolute, gradient relative to max|ref grad|


def _noisy_pair(shape, g, lo=0.0, span=1.0):
    img = torch.rand(shape, generator=g) * span + lo
    gt = (img + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    return img, gt


def ssim_inputs(case):
    """(img, gt, tie mask or None) of one named case.  The shapes use the inputs of
    test_l1_ssim_matches_oracle_fp64; out_of_range has img in [-0.3, 1.6] (the render is unclamped
    when no exposure is trained); ties has img == gt == 0 on one block (alpha-masked sky) and
    img == gt, random, on another; the flat cases are constant planes."""
    if case in FLAT_CASES:
        a, b = FLAT_CASES[case]
        return torch.full(EDGE_SHAPE, a), torch.full(EDGE_SHAPE, b), None
    if case == "out_of_range":
        img, gt = _noisy_pair(EDGE_SHAPE, torch.Generator().manual_seed(21), -0.3, 1.9)
        return img, gt, None
    if case == "ties":
        img, gt = _noisy_pair(EDGE_SHAPE, torch.Generator().manual_seed(22))
        img[:, :30, :50] = 0.0
        gt[:, :30, :50] = 0.0
        gt[:, 40:, 70:] = img[:, 40:, 70:]
        tie = img == gt
        assert bool(tie[:, :30, :50].all()) and bool(tie[:, 40:, 70:].all())
        return img, gt, tie
    shape = tuple(int(v) for v in case.split("x"))
    img, gt = _noisy_pair(shape, torch.Generator().manual_seed(sum(shape)))
    return img, gt, None


def l1_ssim_ref(img, gt, up=SSIM_UP, dtype=torch.float64):
    """(L1, SSIM, d(up[0] L1 + up[1] SSIM)/dimg) of train_ref's torch formulation."""
    x = img.detach().clone().to(dtype).requires_grad_(True)
    y = gt.detach().to(dtype)
    l1, s = TR.l1(x, y), TR.ssim(x, y)
    (up[0] * l1 + up[1] * s).backward()
    return float(l1.detach()), float(s.detach()), x.grad


# ---- depth losses --------------------------------------------------------------------------------
# kDepthPerBlock = 4096 elements per block (float4 per thread, the tail by scalar loads); the
# 1024-thread finalize takes a second trip above 1024 blocks: 2049 x 2049 is 1026 blocks.
DEPTH_SHAPES = [(1, 1, n) for n in (1, 2, 3, 5, 4095, 4096, 4097)] + [(1, 2049, 2049)]


def depth_inputs(shape, depth_only=False, seed=0):
    """(invd, mono, mask): mono == invd on the first 3 elements (sgn(0), the clamp's bound), the
    mask a mix of 0, 1 and 0.5; depth_only: mono zero on 60% of the elements (a LiDAR-like map)."""
    g = torch.Generator().manual_seed(31 + seed + 7 * shape[-1] + shape[-2])
    invd = torch.rand(shape, generator=g)
    mono = invd * (1 + 0.1 * torch.randn(shape, generator=g))
    if depth_only:
        mono = mono * (torch.rand(shape, generator=g) < 0.4).float()
    mono.view(-1)[:3] = invd.view(-1)[:3]
    mask = torch.tensor([0.0, 1.0, 1.0, 0.5])[torch.randint(0, 4, shape, generator=g)]
    return invd, mono, mask


def depth_l1_expr(x, mono, mask, w):
    """train_single.py:138-140."""
    d = x - mono
    return w * torch.abs(d * mask if mask is not None else d).mean()


def depth_only_expr(x, mono, mask, w, a):
    """train_single.py:152-156: (loss, pure, dens)."""
    d = x - mono
    pure = torch.abs(d * mask if mask is not None else d).mean()
    dens = (mono - x).clamp(min=0).mean()
    return w * (a * dens + (1 - a) * pure), pure, dens


def to64(t):
    return None if t is None else t.double()


# ---- the image side composed ---------------------------------------------------------------------
IMAGE_SIDE_SIZES = [(189, 251), (409, 643)]  # (H, W): 251 x 189, and 643 x 409 = 262,987 px, above the exposure cap
LAMBDA_DSSIM, DEPTH_W = 0.2, 0.7


def image_side_inputs(H, W):
    """Leaves color (3, H, W) in [-0.1, 1.3], E, invd; constants gt, an alpha mask (1 with a zero
    block and a 0.5 band), mono and its mask.  gt is zero on part of the zero block (exact ties of
    the L1 sign); elsewhere it stays 1e-4 clear of the exposed image, so that fp32 and fp64 agree on
    sgn(img - gt)."""
    g = torch.Generator().manual_seed(500 * H + W)
    color = torch.rand(3, H, W, generator=g) * 1.4 - 0.1
    E = torch.eye(3, 4) + 0.1 * torch.randn(3, 4, generator=g)
    color = _off_the_clamp_edges(color, E)
    alpha = torch.ones(1, H, W)
    alpha[:, H // 5:H // 2, W // 4:W // 2] = 0.0
    alpha[:, -H // 4:-H // 8, :] = 0.5
    img = exposure_pre(color.double(), E.double()).clamp(0, 1) * alpha.double()
    gt = (img + 0.1 * torch.randn(3, H, W, generator=g).double()).clamp(0, 1).float()
    gt[:, H // 5:H // 3, W // 4:W // 2] = 0.0
    d = gt.double() - img
    close = (d != 0) & (d.abs() < 1e-4)
    gt = torch.where(close, (img + 2e-3).float(), gt)
    d = gt.double() - img
    assert not bool(((d != 0) & (d.abs() < 1e-4)).any())
    assert bool((d == 0).any())
    invd, mono, dmask = depth_inputs((1, H, W), seed=3)
    return dict(color=color, E=E, invd=invd, gt=gt, alpha=alpha, mono=mono, dmask=dmask)


def image_side_ref(p, dtype=torch.float64):
    """loss, color.grad, invd.grad, E.grad and sum|terms| per E.grad entry of
    exposure -> * alpha -> photo loss + depth L1, in torch."""
    color, E, invd = (p[k].detach().clone().to(dtype).requires_grad_(True) for k in ("color", "E", "invd"))
    pre = exposure_pre(color, E)
    out = pre.clamp(0, 1)
    out.retain_grad()
    img = out * p["alpha"].to(dtype)
    loss = TR.photo_loss(img, p["gt"].to(dtype), LAMBDA_DSSIM) + \
        depth_l1_expr(invd, p["mono"].to(dtype), p["dmask"].to(dtype), DEPTH_W)
    loss.backward()
    passes = ((pre >= 0) & (pre <= 1)).detach()
    terms = exposure_terms(p["color"], out.grad.double() * passes)
    return float(loss.detach()), color.grad, invd.grad, E.grad, terms
