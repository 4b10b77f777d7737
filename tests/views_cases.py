"""Inputs of the training-view tests (tests/test_views_cpu.py, tests/test_gpu_views.py): seeded images
for the Lanczos resize and compact views for the expansion.  Every case is a few kilopixels."""
from __future__ import annotations

import numpy as np

# (H, W) -> (h, w); each for C = 1 and 3
LANCZOS_SIZES = [
    ((48, 64), (15, 20)),
    ((97, 131), (48, 65)),      # odd W * C: row starts off a 4-byte boundary
    ((64, 64), (64, 32)),       # vertical pass skipped
    ((64, 64), (32, 64)),       # horizontal pass skipped
    ((40, 50), (80, 75)),       # upscale
    ((33, 200), (5, 7)),        # support clipped at both ends
    ((7, 5), (1, 1)),
    ((1, 1), (3, 3)),
    ((256, 300), (31, 299)),
    ((300, 17), (37, 16)),
    ((400, 416), (200, 208)),   # exactly 2x: 13 taps
    ((24, 1000), (24, 125)),    # 8x: 49 taps
    # beyond the issue's table: a source row segment longer than the horizontal kernel's LDS stage
    # (it is then staged in several pieces), and more than one 256-pixel block per output row
    ((2, 9000), (2, 24)),
    ((3, 1300), (5, 600)),
]


def lanczos_image(H, W, C, seed):
    """Noise over a smooth ramp; half of the image is hard 0 / 255 blocks, so that the filter's
    overshoot reaches both sides of the clip."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    by, bx = np.meshgrid(np.arange(H) // 5, np.arange(W) // 7, indexing="ij")
    blocks = (((by + bx) % 2) * 255).astype(np.uint8)
    half = np.zeros((H, W), bool)
    half[:, W // 2:] = True
    if W == 1:
        half[:] = False
    img[half] = blocks[half][:, None]
    return img if C == 3 else img[..., 0]


def lanczos_cases():
    out = []
    for n, ((H, W), (h, w)) in enumerate(LANCZOS_SIZES):
        for C in (1, 3):
            out.append(dict(name=f"{H}x{W}_to_{h}x{w}_c{C}", image=lanczos_image(H, W, C, 100 + n), size=(w, h)))
    return out


def _view(name, h, w, seed, mask=False, depth=None, scale=0.0, offset=0.0, depth_only=False, test_half=None,
          depth_valid="alpha"):
    rng = np.random.default_rng(seed)
    c = dict(name=name, size=(w, h), scale=scale, offset=offset, depth_only=depth_only, test_half=test_half,
             depth_valid=depth_valid, image=None, mask=None, u16=None)
    if not depth_only:
        c["image"] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        c["image"].reshape(-1)[:3] = (0, 1, 254)
        c["image"].reshape(-1)[-1] = 255
    if mask:
        m = rng.choice(np.array([0, 1, 2, 127, 128, 254, 255], np.uint8), (h, w))
        m.reshape(-1)[:min(4, h * w)] = np.array([255, 254, 1, 0], np.uint8)[:h * w]
        c["mask"] = m
    if depth is not None:
        dh, dw = depth
        u = rng.integers(0, 65536, (dh, dw)).astype(np.int32)
        u[rng.uniform(size=u.shape) < 0.2] = 0  # no hit
        u.reshape(-1)[:min(2, dh * dw)] = np.array([65535, 0])[:dh * dw]
        c["u16"] = u
    return c


def expand_cases():
    return [
        _view("plain", 12, 20, 1),
        _view("mask", 12, 20, 2, mask=True),
        _view("depth_same_res", 12, 20, 3, depth=(12, 20), scale=0.37, offset=0.011),
        _view("mask_depth_down", 48, 64, 4, mask=True, depth=(96, 128), scale=0.8, offset=-0.25),  # negatives
        _view("depth_ragged", 37, 41, 5, mask=True, depth=(50, 70), scale=1.3, offset=-0.6, depth_valid="alpha_and_hit"),
        _view("depth_up", 45, 61, 6, depth=(20, 30), scale=0.05, offset=0.002, depth_valid="alpha_and_hit"),
        _view("scale_zero", 9, 13, 7, mask=True, depth=(9, 13), scale=0.0, offset=0.5),
        _view("scale_negative", 9, 13, 8, depth=(9, 13), scale=-1.0, offset=0.5),
        _view("depth_only", 16, 24, 9, depth=(16, 24), scale=0.6, offset=0.01, depth_only=True),
        _view("depth_only_mask", 11, 17, 10, mask=True, depth=(22, 34), scale=0.6, offset=-0.2, depth_only=True,
              depth_valid="alpha_and_hit"),
        _view("half_left_odd", 10, 21, 11, mask=True, test_half="left"),
        _view("half_right_odd", 10, 21, 12, depth=(10, 21), scale=0.4, offset=0.0, test_half="right"),
        _view("one_pixel", 1, 1, 13, mask=True, depth=(1, 1), scale=0.5, offset=0.1),
        _view("ragged_tail", 7, 9, 14, mask=True, depth=(5, 3), scale=0.9, offset=-0.3),  # W * H = 63
        _view("width_one", 5, 1, 15, depth=(3, 1), scale=0.9, offset=0.0, test_half="left"),
    ]
