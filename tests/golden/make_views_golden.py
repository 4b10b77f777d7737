"""Generate tests/golden/views.npz from the reference's own PILtoTorch (build container only).

utils/general_utils.py:22-29 is what turns a decoded image or mask into the float32 tensor a Camera
holds: Image.resize(resolution, Image.LANCZOS) when the size differs, then / 255.0 and channels
first.  The module is loaded from the reference by path and run here on six small seeded inputs.

Stored per case k: in_k (H, W[, 3]) uint8, size_k = (w, h), out_k (C, h, w) float32: PILtoTorch's
return value.  out_k * 255 is integral, so the fixture pins the resize bit for bit and the division.

Nothing from the reference is copied; only numbers are kept.
Usage:  python tests/golden/make_views_golden.py --ref <reference checkout>
"""
from __future__ import annotations

import argparse
import importlib.util
import os

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))

# (H, W, C) -> (w, h)
CASES = [((37, 53, 3), (26, 18)),     # both passes, odd row starts
         ((40, 44, 1), (22, 20)),     # a mask at exactly 2x
         ((12, 15, 3), (31, 25)),     # upscale
         ((20, 24, 3), (24, 20)),     # same size: PILtoTorch does not resize
         ((16, 96, 3), (12, 16)),     # horizontal pass only, 8x
         ((90, 9, 1), (9, 11))]       # vertical pass only


def inputs():
    rng = np.random.default_rng(41)
    out = []
    for (H, W, C), size in CASES:
        img = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
        img[:, W // 2:] = ((((np.arange(H)[:, None] // 3) + (np.arange(W - W // 2)[None, :] // 4)) % 2) * 255
                           ).astype(np.uint8)[..., None]  # hard edges: the filter overshoots into the clip
        out.append((img if C == 3 else img[..., 0], size))
    return out


def import_reference(ref):
    path = os.path.join(ref, "utils", "general_utils.py")
    spec = importlib.util.spec_from_file_location("ref_general_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout")
    M = import_reference(ap.parse_args().ref)
    out = {"n": np.int32(len(CASES))}
    for k, (img, size) in enumerate(inputs()):
        t = M.PILtoTorch(Image.fromarray(img), size)
        out.update({f"in_{k}": img, f"size_{k}": np.array(size, np.int32), f"out_{k}": t.numpy().astype(np.float32)})
        assert out[f"out_{k}"].shape[1:] == (size[1], size[0])
    path = os.path.join(OUT, "views.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < os.path.getsize(os.path.join(OUT, "depth_encode.npz"))
    print(f"{path}: {os.path.getsize(path)} bytes, {len(CASES)} cases")


if __name__ == "__main__":
    main()
