"""Numpy restatements of include/gsr_views.h: Pillow's 8-bit Lanczos resize in integers, and the
expansion of a compact training view (RGB8, mask8, depth16) into the float32 planes the reference's
Camera holds (scene/cameras.py:47-88), every float32 operation rounded once, in the stated order.

The `mutant` arguments switch one rule off each; tests/test_views_cpu.py shows that every one of them
is caught by the cases of tests/views_cases.py (profiles/r22_views_mutation_check.txt)."""
from __future__ import annotations

import math

import numpy as np

PRECISION_BITS = 22
F32 = np.float32


def _lanczos(t: float) -> float:
    def sinc(x):
        if x == 0.0:
            return 1.0
        x = x * math.pi
        return math.sin(x) / x
    return sinc(t) * sinc(t / 3.0) if -3.0 <= t < 3.0 else 0.0


def lanczos_coeffs(in_size: int, out_size: int, mutant: str = ""):
    """(ksize, xmin[out], count[out], coeff[out, ksize] int32) of one axis."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    xmin_a, cnt_a = np.zeros(out_size, np.int32), np.zeros(out_size, np.int32)
    coeff = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + (0.0 if mutant == "xmin_trunc" else 0.5)), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = [_lanczos((x + xmin - center + 0.5) / fs) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            if v < 0 and mutant != "round_neg":
                coeff[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5)
            else:
                coeff[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5)
        xmin_a[xx], cnt_a[xx] = xmin, n
    return ksize, xmin_a, cnt_a, coeff


def _pass(img: np.ndarray, axis: int, out_size: int, mutant: str, keep_wide: bool = False):
    """One pass along `axis` of an (H, W, C) array; int64 accumulation."""
    _, xmin, cnt, coeff = lanczos_coeffs(img.shape[axis], out_size, mutant)
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.zeros((out_size,) + src.shape[1:], np.int64)
    start = 0 if mutant == "no_half" else 1 << (PRECISION_BITS - 1)
    for xx in range(out_size):
        n = int(cnt[xx])
        acc = np.tensordot(coeff[xx, :n].astype(np.int64), src[xmin[xx]:xmin[xx] + n], axes=(0, 0)) + start
        out[xx] = acc >> PRECISION_BITS
    if not keep_wide:
        out = np.clip(out, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_lanczos_ref(image: np.ndarray, size, mutant: str = "") -> np.ndarray:
    """image: (H, W) or (H, W, 3) uint8; size: (w, h).  Image.resize(size, Image.LANCZOS)."""
    a = np.asarray(image)
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    img = a.reshape(a.shape[0], a.shape[1], -1)
    w, h = int(size[0]), int(size[1])
    order = [(1, w), (0, h)]
    if mutant == "vertical_first":
        order.reverse()
    for n, (axis, out) in enumerate(order):
        if img.shape[axis] != out:
            img = _pass(img, axis, out, mutant, keep_wide=(mutant == "no_u8_between" and n == 0))
    return np.clip(img, 0, 255).astype(np.uint8).reshape((h, w) + a.shape[2:])


# ---- the float32 linear resize (OpenCV's INTER_LINEAR rule as include/gsr_views.h states it) ------------

def linear_taps(in_size: int, out_size: int):
    """(i[out] int32, f[out] float32) of one axis."""
    scale = float(in_size) / float(out_size)
    idx, frac = np.zeros(out_size, np.int32), np.zeros(out_size, F32)
    for d in range(out_size):
        f = F32((d + 0.5) * scale - 0.5)
        i = int(math.floor(f))
        f = F32(f - F32(i))
        if i < 0:
            i, f = 0, F32(0)
        if i >= in_size - 1:
            i, f = in_size - 1, F32(0)
        idx[d], frac[d] = i, f
    return idx, frac


def resize_linear_ref(S: np.ndarray, size) -> np.ndarray:
    """S: (H, W) float32; size: (w, h)."""
    S = np.asarray(S, F32)
    H, W = S.shape
    w, h = int(size[0]), int(size[1])
    ix, fx = linear_taps(W, w)
    iy, fy = linear_taps(H, h)
    ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
    a1, a0 = fx[None, :], (F32(1) - fx)[None, :]
    b1, b0 = fy[:, None], (F32(1) - fy)[:, None]
    with np.errstate(invalid="ignore"):
        h0 = (a0 * S[iy][:, ix]).astype(F32) + (a1 * S[iy][:, ix1]).astype(F32)
        h1 = (a0 * S[iy1][:, ix]).astype(F32) + (a1 * S[iy1][:, ix1]).astype(F32)
        out = (b0 * h0.astype(F32)).astype(F32) + (b1 * h1.astype(F32)).astype(F32)
    return out.astype(F32)


def expand_ref(image=None, mask=None, u16=None, scale=0.0, offset=0.0, size=None, depth_only=False, test_half=None,
               depth_valid="alpha", mutant: str = "") -> dict:
    """The planes of one view.  image (h, w, 3) uint8 or None (depth-only), mask (h, w) uint8 or None,
    u16 (dh, dw) integers 0..65535 or None; size (w, h) when there is no image.  Returns
    original_image (3, h, w), alpha_mask (1, h, w), and invdepthmap / depth_mask (1, h, w) or None."""
    if image is not None:
        h, w = image.shape[:2]
    else:
        w, h = size
    alpha = np.ones((h, w), F32) if mask is None else np.asarray(mask, np.uint8).astype(F32) / F32(255.0)
    if mutant == "reciprocal" and mask is not None:
        alpha = np.asarray(mask, np.uint8).astype(F32) * F32(1.0 / 255.0)
    alpha = alpha.astype(F32).copy()
    if test_half == "left":
        alpha[:, :w // 2] = 0
    elif test_half == "right":
        alpha[:, w // 2:] = 0
    if depth_only or image is None:
        rgb = np.zeros((3, h, w), F32)
    else:
        u8 = np.asarray(image, np.uint8).astype(F32)
        v = u8 * F32(1.0 / 255.0) if mutant == "reciprocal" else u8 / F32(255.0)
        rgb = np.minimum(np.maximum(v.astype(F32), F32(0)), F32(1)).transpose(2, 0, 1)
    out = {"original_image": (rgb * alpha[None]).astype(F32), "alpha_mask": alpha[None], "invdepthmap": None,
           "depth_mask": None}
    if u16 is not None and scale > 0:
        m = np.asarray(u16).astype(np.int64).astype(F32) / F32(65536.0)
        s = ((m * F32(scale)).astype(F32) + F32(offset)).astype(F32)
        if mutant == "clip_first":
            s = np.maximum(s, F32(0))
        d = resize_linear_ref(s, (w, h))
        d = np.where(d < 0, F32(0), d).astype(F32)
        dm = alpha.copy()
        if depth_valid == "alpha_and_hit":
            dm[d == 0] = 0
        out["invdepthmap"], out["depth_mask"] = d[None], dm[None]
    return out
