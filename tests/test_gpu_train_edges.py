"""The image side of a training iteration (csrc/loss.hip: exposure affine, alpha mask, L1 + SSIM,
masked inverse-depth L1, depth-only loss) against fp64 torch at the sizes and values where such
kernels go wrong: one pixel, one pixel past a block, past the exposure grid's cap (a second and a
third grid-stride trip), images smaller than the 11-tap SSIM window, widths and heights that are no
multiple of the 64-wide strips, values outside [0, 1], flat planes, exact ties of sgn and of the
clamp, fractional masks and operands that start off a 16-byte boundary.  Inputs and references:
tests/train_edge_cases.py (tests/test_train_cpu.py checks their conditioning).

Bars: those of tests/test_gpu_train.py (values 2e-6, gradients 1e-5 of max|ref grad|, exposure out
and dcolor 1e-6, depth values 2e-6 relative, depth gradients bit-identical to torch autograd on the
device), and for the exposure gradient dE the derived summation bound 4e-6 * sum|terms|
(train_edge_cases.EXPOSURE_DE_BOUND).  Recorded margins: profiles/r14_train_edge_margins.jsonl.
"""
from __future__ import annotations

import contextlib
import functools

import pytest
import torch

import train_edge_cases as EC
from helpers import record_margins

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---- exposure ------------------------------------------------------------------------------------
def _exposure_on_device(color, E, up):
    from gs_train import apply_exposure
    c = color.to(DEV).requires_grad_(True)
    e = E.to(DEV).requires_grad_(True)
    out = apply_exposure(c, e)
    (out * up.to(DEV)).sum().backward()
    return out.detach().double().cpu(), c.grad.double().cpu(), e.grad.double().cpu()


@pytest.mark.parametrize("localised", [False, True])
@pytest.mark.parametrize("size", EC.EXPOSURE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exposure_matches_fp64_at_ragged_sizes(size, localised):
    """gs_train.apply_exposure and its backward at one pixel, around one block, at the last
    one-trip size of the capped grid, one pixel into the second trip and in a partly filled third
    one.  dE is held to the summation bound: with the localised upstream (zero but for the first 3
    and last 300 pixels of a plane) one lost or doubled tail pixel is thousands of times the bar."""
    color, E, up = EC.exposure_inputs(*size, localised)
    out_ref, dc_ref, dE_ref, terms = EC.exposure_ref(color, E, up)
    out, dc, dE = _exposure_on_device(color, E, up)
    e_out = (out - out_ref).abs().max().item()
    e_dc = (dc - dc_ref).abs().max().item()
    frac = ((dE - dE_ref).abs() / (EC.EXPOSURE_DE_BOUND * terms).clamp_min(1e-300)).max().item()
    print(f"exposure {size} localised={localised}: out {e_out:.3g} dcolor {e_dc:.3g} dE / bound {frac:.3g}")
    record_margins(f"exposure_{size[0]}x{size[1]}_{'localised' if localised else 'dense'}", out=e_out, dcolor=e_dc,
                   dE_over_bound=frac)
    assert e_out <= 1e-6
    assert e_dc <= 1e-6
    assert bool(((dE - dE_ref).abs() <= EC.EXPOSURE_DE_BOUND * terms).all()), frac


@pytest.mark.parametrize("size", [(1, 257), (5, 52429)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_exposure_clamp_passes_gradient_at_exact_zero_and_one(size):
    """The exact identity exposure over colours from {-0.5, 0, 0.25, 1, 1.5}: pre-clamp values of
    exactly 0 and 1 pass the gradient (torch.clamp), the others inside do, those outside do not --
    dcolor equals the upstream or zero, exactly."""
    color, E, up = EC.exposure_tie_inputs(*size)
    for v in EC.TIE_COLOURS:
        assert bool((color == v).any()), v
    out_ref, dc_ref, dE_ref, terms = EC.exposure_ref(color, E, up)
    out, dc, dE = _exposure_on_device(color, E, up)
    inside = (color == 0.0) | (color == 0.25) | (color == 1.0)
    want = torch.where(inside, up, torch.zeros_like(up)).double()
    assert torch.equal(dc_ref, want)  # the fp64 reference sees the same pre-clamp values
    assert torch.equal(out, out_ref)
    assert torch.equal(dc, want)
    assert bool(((dE - dE_ref).abs() <= EC.EXPOSURE_DE_BOUND * terms).all())
    record_margins(f"exposure_ties_{size[0]}x{size[1]}", dcolor=(dc - want).abs().max().item(),
                   dE_over_bound=((dE - dE_ref).abs() / (EC.EXPOSURE_DE_BOUND * terms).clamp_min(1e-300)).max().item())


# ---- L1 + SSIM -----------------------------------------------------------------------------------
@contextlib.contextmanager
def ssim_kernel(tiled):
    """gsr_set_ssim_kernel: 0 the streaming gradient kernel, 1 the 64 x 16 tile kernel."""
    from gs_train._native import lib
    prev = lib().gsr_set_ssim_kernel(tiled)
    assert prev >= 0, prev
    try:
        yield
    finally:
        lib().gsr_set_ssim_kernel(prev)


@functools.lru_cache(maxsize=None)
def _ssim_case(case):
    img, gt, tie = EC.ssim_inputs(case)
    return img, gt, tie, EC.l1_ssim_ref(img, gt)


def _l1_ssim_paths(img, gt, up=EC.SSIM_UP):
    """{path: (L1, SSIM, gradient)} of the four ways the loss is evaluated: l1_ssim with a gradient
    (forward with the SSIM gradient field, elementwise backward), gsr_l1_ssim_backward (direct),
    photo_loss (lambda = -up[1]; also its loss value) and the forward alone."""
    from gs_train import l1_ssim, photo_loss
    from gs_train._native import lib, ptr, stream
    img, gt = img.to(DEV), gt.to(DEV)
    upt = torch.tensor(up, device=DEV)
    C, H, W = img.shape
    res = {}
    x = img.clone().requires_grad_(True)
    v = l1_ssim(x, gt)
    (v * upt).sum().backward()
    res["map"] = (v[0].item(), v[1].item(), x.grad)
    direct = torch.empty_like(img)
    assert lib().gsr_l1_ssim_backward(ptr(img), ptr(gt), C, H, W, ptr(upt), ptr(direct), stream(img.device)) == 0
    res["direct"] = (None, None, direct)
    if up[0] + -up[1] == 1.0:
        x = img.clone().requires_grad_(True)
        loss, l1, s = photo_loss(x, gt, -up[1])
        loss.backward()
        res["photo"] = (l1.item(), s.item(), x.grad, loss.item())
    with torch.no_grad():
        v0 = l1_ssim(img, gt)
    res["forward"] = (v0[0].item(), v0[1].item(), None)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("tiled", [0, 1], ids=["streaming", "tiled"])
@pytest.mark.parametrize("case", EC.SSIM_CASES)
def test_l1_ssim_matches_fp64_at_small_ragged_and_tied_inputs(case, tiled):
    """Every way the loss is evaluated, with both SSIM kernels, against fp64: images smaller than
    the window ((1,1,1), (1,5,9), (1,10,70), (3,11,11)), widths and heights one off the 64-wide
    strips, an unclamped render and regions where img == gt."""
    img, gt, tie, (l1_ref, s_ref, g_ref) = _ssim_case(case)
    gmax = g_ref.abs().max().item()
    with ssim_kernel(tiled):
        res = _l1_ssim_paths(img, gt)
        tied = _l1_ssim_paths(img, gt, up=(1.0, 0.0)) if tie is not None else None
    worst_v, worst_g = 0.0, 0.0
    for path, r in res.items():
        if r[0] is not None:
            ev = max(abs(r[0] - l1_ref), abs(r[1] - s_ref))
            if path == "photo":
                ev = max(ev, abs(r[3] - (EC.SSIM_UP[0] * l1_ref - EC.SSIM_UP[1] * (1 - s_ref))))
            worst_v = max(worst_v, ev)
            print(f"{case} tiled={tiled} {path}: values {ev:.3g}")
            assert ev <= EC.VALUE_BAR, (path, ev)
        if r[2] is not None:
            eg = (r[2].double().cpu() - g_ref).abs().max().item()
            worst_g = max(worst_g, eg / gmax)
            print(f"{case} tiled={tiled} {path}: gradient {eg / gmax:.3g} of max|ref|")
            assert eg <= EC.GRAD_BAR * gmax, (path, eg / gmax)
    record_margins(f"l1_ssim_{case}_{'tiled' if tiled else 'streaming'}", values=worst_v, grad_rel=worst_g)
    if tie is not None:  # sgn(0) = 0: with the upstream (1, 0) the gradient vanishes where img == gt
        for path in ("map", "direct"):
            dx = tied[path][2].cpu()
            assert bool((dx[tie] == 0).all()), path
            assert bool((dx[~tie] != 0).all()), path


@functools.lru_cache(maxsize=None)
def _flat_case(case):
    """A flat plane is ill-conditioned in fp32 (sigma^2 = E[x^2] - mu^2 cancels against C2 = 9e-4),
    so the bar is set by the fp32 torch reference's own distance from fp64, measured here."""
    img, gt, _ = EC.ssim_inputs(case)
    ref = EC.l1_ssim_ref(img, gt)
    f32 = EC.l1_ssim_ref(img, gt, dtype=torch.float32)
    dist = (abs(f32[0] - ref[0]), abs(f32[1] - ref[1]), (f32[2].double() - ref[2]).abs().max().item())
    return img, gt, ref, dist


@pytest.mark.parametrize("tiled", [0, 1], ids=["streaming", "tiled"])
@pytest.mark.parametrize("case", list(EC.FLAT_CASES))
def test_l1_ssim_on_flat_planes(case, tiled):
    """Constant planes (0.7 against 0.4, and equal planes whose true gradient is 0): the kernels may
    be at most 4x as far from fp64 as the fp32 torch reference is (the margin for ill-conditioned
    rows, as in test_gpu_shapes.py), with a floor of 1e-7 per value and 1e-7 * (0.8 / n) per
    gradient element; 0 against 0 gives L1 = 0, SSIM = 1 and a zero gradient exactly."""
    img, gt, (l1_ref, s_ref, g_ref), (d_l1, d_s, d_g) = _flat_case(case)
    n = img.numel()
    bars = (max(4 * d_l1, 1e-7), max(4 * d_s, 1e-7), max(4 * d_g, 1e-7 * 0.8 / n))
    with ssim_kernel(tiled):
        res = _l1_ssim_paths(img, gt)
    ratios = {}
    for path, r in res.items():
        if r[0] is not None:
            ratios[f"l1_{path}"] = abs(r[0] - l1_ref) / bars[0]
            ratios[f"ssim_{path}"] = abs(r[1] - s_ref) / bars[1]
            if case == "flat_0_0":
                assert r[0] == 0.0 and r[1] == 1.0, (path, r[:2])
        if r[2] is not None:
            ratios[f"grad_{path}"] = (r[2].double().cpu() - g_ref).abs().max().item() / bars[2]
            if case == "flat_0_0":
                assert bool((r[2] == 0).all()), path
    print(f"{case} tiled={tiled}: fp32 torch distance (L1, SSIM, grad) {d_l1:.3g} {d_s:.3g} {d_g:.3g}; "
          f"share of each bar {ratios}")
    record_margins(f"l1_ssim_{case}_{'tiled' if tiled else 'streaming'}", ref32_l1=d_l1, ref32_ssim=d_s, ref32_grad=d_g,
                   **{f"share_{k}": v for k, v in ratios.items()})
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)


@pytest.mark.parametrize("tiled", [0, 1], ids=["streaming", "tiled"])
@pytest.mark.parametrize("case", ["3x65x63", "1x1x1", "ties"])
def test_l1_ssim_map_backward_off_a_16_byte_boundary(case, tiled):
    """gsr_l1_ssim_backward_from_map takes its scalar path when a pointer is not 16-byte aligned:
    img, gt, the gradient field and the output placed 4 bytes past such a boundary give the bits of
    the aligned (float4) run."""
    from gs_train._native import lib, ptr, stream
    img, gt, _, _ = _ssim_case(case)
    C, H, W = img.shape
    n = img.numel()
    L = lib()
    up = torch.tensor(EC.SSIM_UP, device=DEV)
    scratch = torch.empty(max(8, L.gsr_l1_ssim_scratch_bytes(C, H, W)), dtype=torch.uint8, device=DEV)
    got = {}
    with ssim_kernel(tiled):
        for off in (0, 1):
            def place(src=None):
                store = torch.zeros(n + 4, device=DEV)
                t = store[off:off + n].view(C, H, W)
                if src is not None:
                    t.copy_(src)
                assert t.data_ptr() % 16 == 4 * off
                return t
            x, y, gmap, dx = place(img), place(gt), place(), place()
            out = torch.empty(2, device=DEV)
            s = stream(x.device)
            assert L.gsr_l1_ssim_forward_with_map(ptr(x), ptr(y), C, H, W, ptr(scratch), ptr(out), ptr(gmap), s) == 0
            assert L.gsr_l1_ssim_backward_from_map(ptr(x), ptr(y), ptr(gmap), C, H, W, ptr(up), ptr(dx), s) == 0
            torch.cuda.synchronize()
            got[off] = (out.clone(), gmap.clone(), dx.clone())
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a, b)
    assert bool(got[0][2].abs().sum() > 0)


# ---- depth losses --------------------------------------------------------------------------------
def _depth_id(shape):
    return "x".join(map(str, shape))


def _rel(a, ref):
    return abs(a - ref) / abs(ref) if ref != 0 else (0.0 if a == 0 else float("inf"))


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("shape", EC.DEPTH_SHAPES, ids=_depth_id)
def test_depth_l1_at_block_edges_and_fractional_masks(shape, masked):
    """gs_train.loss.depth_l1_loss below one float4, around one 4096-element block and above 1024
    blocks (the finalize's second trip), with a mask of 0, 1 and 0.5: the gradient bit-identical
    to torch autograd on the device, the value within 2e-6 (relative) of fp64."""
    from gs_train.loss import depth_l1_loss
    invd, mono, mask = EC.depth_inputs(shape)
    mask = mask if masked else None
    w = 0.73
    ref = EC.depth_l1_expr(invd.double(), mono.double(), EC.to64(mask), w).item()
    invd, mono = invd.to(DEV), mono.to(DEV)
    mask = mask.to(DEV) if masked else None
    a = invd.clone().requires_grad_(True)
    la = depth_l1_loss(a, mono, mask, w)
    la.backward()
    b = invd.clone().requires_grad_(True)
    EC.depth_l1_expr(b, mono, mask, w).backward()
    rel = _rel(la.item(), ref)
    print(f"depth_l1 {shape} masked={masked}: value rel {rel:.3g}")
    record_margins(f"depth_l1_{_depth_id(shape)}_{'mask' if masked else 'nomask'}", value_rel=rel)
    assert torch.equal(a.grad, b.grad)
    assert rel <= 2e-6


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("shape", EC.DEPTH_SHAPES, ids=_depth_id)
def test_depth_only_loss_at_block_edges_and_fractional_masks(shape, masked):
    """The same for gs_train.loss.depth_only_loss over a map that is zero on 60% of its elements:
    loss, pure and dens within 2e-6 (relative) of fp64, the gradient bit-identical."""
    from gs_train.loss import depth_only_loss
    invd, mono, mask = EC.depth_inputs(shape, depth_only=True)
    mask = mask if masked else None
    w, a = 0.61, 0.9
    refs = [v.item() for v in EC.depth_only_expr(invd.double(), mono.double(), EC.to64(mask), w, a)]
    invd, mono = invd.to(DEV), mono.to(DEV)
    mask = mask.to(DEV) if masked else None
    x = invd.clone().requires_grad_(True)
    got = depth_only_loss(x, mono, mask, w, a)
    got[0].backward()
    y = invd.clone().requires_grad_(True)
    EC.depth_only_expr(y, mono, mask, w, a)[0].backward()
    rels = [_rel(g.item(), r) for g, r in zip(got, refs)]
    print(f"depth_only {shape} masked={masked}: loss, pure, dens rel {rels}")
    record_margins(f"depth_only_{_depth_id(shape)}_{'mask' if masked else 'nomask'}", loss_rel=rels[0],
                   pure_rel=rels[1], dens_rel=rels[2])
    assert torch.equal(x.grad, y.grad)
    assert max(rels) <= 2e-6


def test_depth_losses_on_slices_of_stacked_maps():
    """monos and masks as one stacked (3, 1, 37, 53) tensor each: 37 * 53 is odd, so the slices of
    views 1 and 2 start off a 16-byte boundary.  The C entry points refuse such arrays (they load
    float4); the wrappers copy them, and every view gives the bits of torch autograd."""
    from gs_train._native import lib, ptr, stream
    from gs_train.loss import depth_l1_loss, depth_only_loss
    V, shape = 3, (1, 37, 53)
    per_view = [EC.depth_inputs(shape, depth_only=True, seed=k) for k in range(V)]
    invds = [p[0].to(DEV) for p in per_view]
    monos = torch.stack([p[1] for p in per_view]).to(DEV)
    masks = torch.stack([p[2] for p in per_view]).to(DEV)
    assert monos[1].data_ptr() % 16 != 0 and masks[2].data_ptr() % 16 != 0 and monos[1].is_contiguous()
    L = lib()
    n = invds[1].numel()
    scratch = torch.empty(max(16, int(L.gsr_depth_only_scratch_bytes(n))), dtype=torch.uint8, device=DEV)
    out = torch.empty(3, device=DEV)
    s = stream(out.device)
    assert L.gsr_depth_l1_forward(ptr(invds[1]), ptr(monos[1]), ptr(masks[1]), n, 0.5, ptr(scratch), ptr(out), s) != 0
    assert L.gsr_depth_only_loss_forward(ptr(invds[1]), ptr(monos[1]), None, n, 0.5, 0.9, ptr(scratch), ptr(out),
                                         s) != 0
    w, a = 0.73, 0.9
    for i in range(V):
        for mask in (masks[i], None):
            x = invds[i].clone().requires_grad_(True)
            lx = depth_l1_loss(x, monos[i], mask, w)
            lx.backward()
            y = invds[i].clone().requires_grad_(True)
            EC.depth_l1_expr(y, monos[i], mask, w).backward()
            ref = EC.depth_l1_expr(invds[i].double(), monos[i].double(), EC.to64(mask), w).item()
            assert torch.equal(x.grad, y.grad), i
            assert _rel(lx.item(), ref) <= 2e-6, i
            x = invds[i].clone().requires_grad_(True)
            got = depth_only_loss(x, monos[i], mask, w, a)
            got[0].backward()
            y = invds[i].clone().requires_grad_(True)
            EC.depth_only_expr(y, monos[i], mask, w, a)[0].backward()
            refs = EC.depth_only_expr(invds[i].double(), monos[i].double(), EC.to64(mask), w, a)
            assert torch.equal(x.grad, y.grad), i
            rels = [_rel(g.item(), r.item()) for g, r in zip(got, refs)]
            record_margins(f"depth_stacked_view{i}_{'mask' if mask is not None else 'nomask'}",
                           l1_rel=_rel(lx.item(), ref), only_rel=max(rels))
            assert max(rels) <= 2e-6, i


# ---- the image side composed ---------------------------------------------------------------------
@pytest.mark.parametrize("size", EC.IMAGE_SIDE_SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_image_side_composed_matches_fp64(size):
    """apply_exposure -> * alpha -> photo_loss(., gt, 0.2) + depth_l1_loss(invd, ., 0.7) and its
    backward through the wrappers, against the same in fp64 torch, at 251 x 189 and at 643 x 409
    (above the exposure grid's cap): a wrong last column or tail pixel moves color.grad, invd.grad
    or E.grad, where an Adam trajectory would normalise it away."""
    from gs_train import apply_exposure, photo_loss
    from gs_train.loss import depth_l1_loss
    p = EC.image_side_inputs(*size)
    loss_ref, dc_ref, di_ref, dE_ref, terms = EC.image_side_ref(p)
    d = {k: v.to(DEV) for k, v in p.items()}
    color, E, invd = (d[k].clone().requires_grad_(True) for k in ("color", "E", "invd"))
    img = apply_exposure(color, E) * d["alpha"]
    loss = photo_loss(img, d["gt"], EC.LAMBDA_DSSIM)[0] + depth_l1_loss(invd, d["mono"], d["dmask"], EC.DEPTH_W)
    loss.backward()
    e_loss = abs(loss.item() - loss_ref)
    e_dc = (color.grad.double().cpu() - dc_ref).abs().max().item() / dc_ref.abs().max().item()
    e_di = (invd.grad.double().cpu() - di_ref).abs().max().item() / di_ref.abs().max().item()
    dE = E.grad.double().cpu()
    frac = ((dE - dE_ref).abs() / (EC.EXPOSURE_DE_BOUND * terms)).max().item()
    print(f"image side {size}: loss {e_loss:.3g} color.grad {e_dc:.3g} invd.grad {e_di:.3g} E.grad / bound {frac:.3g}")
    record_margins(f"image_side_{size[1]}x{size[0]}", loss=e_loss, color_grad_rel=e_dc, invd_grad_rel=e_di,
                   dE_over_bound=frac)
    assert e_loss <= EC.VALUE_BAR
    assert e_dc <= EC.GRAD_BAR
    assert e_di <= EC.GRAD_BAR
    assert bool(((dE - dE_ref).abs() <= EC.EXPOSURE_DE_BOUND * terms).all()), frac
