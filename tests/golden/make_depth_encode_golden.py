"""Generate tests/golden/depth_encode.npz from the reference's own depth conversion (build container only).

The reference's ray caster writes distances in a 3-channel code (DistanceToColor,
render_depth_gaussians.cpp:162-195) and ss_utils/depth_scripts/depth_map_to_distances.py decodes it
(convert_depth_map_to_meters) and makes the 16-bit normalised inverse depth map with its scale and
offset (convert_to_gaussian_splatting_format).  The two Python functions are imported from the
reference and run here, with cv2 (cv2.split is three slices) and read_write_model stubbed.  The C++
half cannot be run, so the BGR images they are given come from this file's own statement of the code
(code_of below): the decode and the normalisation are pinned to the reference, the code is restated.

Stored per case k: mm_k (H, W) float64, the millimetres the code is made of; bgr_k (H, W, 3) uint8;
depth_k, background_k: what convert_depth_map_to_meters returns; and for every setting s of
(min_depth, max_depth) in SETTINGS: u16_k_s, and scale_offset_k_s = (scale, offset).

Nothing from the reference is copied; only numbers are kept.
Usage:  python tests/golden/make_depth_encode_golden.py --ref <reference checkout>
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
SETTINGS = [(0.1, None), (0.5, 300.0), (0.0, None)]


def code_of(mm):
    """(H, W, 3) uint8 BGR of float64 millimetres: val = 0 below 1 mm and above 1048576 mm (and for
    NaN), else (0x40 k << 16) | ((uint32)(mm / 4^k) << 8) with k = 1, 2, 3 for mm <= 65536, <= 262144,
    <= 1048576; R, G, B = bits 16-23, 8-15, 0-7."""
    mm = np.asarray(mm, np.float64)
    val = np.zeros(mm.shape, np.uint32)
    with np.errstate(invalid="ignore"):
        for k, (lo, hi) in enumerate(((1.0, 65536.0), (65536.0, 262144.0), (262144.0, 1048576.0)), start=1):
            m = (mm >= 1.0) & (mm <= hi) & ((mm > lo) | (k == 1))
            units = np.where(m, mm / float(4 ** k), 0.0).astype(np.uint32)
            val = np.where(m, (np.uint32(0x40 * k) << np.uint32(16)) | (units << np.uint32(8)), val)
    return np.stack([val & 0xFF, (val >> 8) & 0xFF, (val >> 16) & 0xFF], -1).astype(np.uint8)


def import_reference(ref):
    cv2 = types.ModuleType("cv2")
    cv2.split = lambda im: (im[..., 0], im[..., 1], im[..., 2])
    sys.modules["cv2"] = cv2
    sys.modules["read_write_model"] = types.ModuleType("read_write_model")
    path = os.path.join(ref, "ss_utils", "depth_scripts", "depth_map_to_distances.py")
    spec = importlib.util.spec_from_file_location("ref_depth_map_to_distances", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs():
    rng = np.random.default_rng(29)
    limits = []
    for v in (1.0, 65536.0, 262144.0, 1048576.0):
        limits += [np.nextafter(v, 0.0), v, np.nextafter(v, np.inf), v - 0.3, v + 0.3]
    steps = [4.0, 7.999, 8.0, 65532.0, 65535.999, 65540.0, 65552.0, 262128.0, 262143.5, 262208.0, 1048512.0, 1048575.0]
    special = [0.0, 0.5, np.nan, -3.0, np.inf, 2e6, 100.0, 104.0, 99.999, 500.0, 299999.0, 300000.0, 300001.0]
    edge = np.array(limits + steps + special, np.float64)
    edge = np.concatenate([edge, np.full(48 - len(edge), 2500.0)]).reshape(4, 12)
    wide = np.exp(rng.uniform(np.log(0.3), np.log(3e6), (70, 130)))
    wide[rng.uniform(size=wide.shape) < 0.15] = 0.0
    near = rng.uniform(200.0, 90000.0, (9, 11))
    one = np.zeros((4, 6))
    one[2, 3] = 7300.0
    two = np.zeros((4, 6))
    two[1, 1] = two[3, 5] = 12344.0
    return [edge, wide, near, np.zeros((5, 7)), one, two, np.full((1, 1), 3000.0), np.full((1, 1), 65536.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout")
    M = import_reference(ap.parse_args().ref)
    out = {"settings": np.array([[a, -1.0 if b is None else b] for a, b in SETTINGS])}
    cases = inputs()
    out["n"] = np.int32(len(cases))
    for k, mm in enumerate(cases):
        bgr = code_of(mm)
        depth, bg = M.convert_depth_map_to_meters(bgr)
        out.update({f"mm_{k}": mm, f"bgr_{k}": bgr, f"depth_{k}": depth.astype(np.float64), f"background_{k}": bg})
        for s, (lo, hi) in enumerate(SETTINGS):
            with np.errstate(divide="ignore"):
                u16, scale, offset = M.convert_to_gaussian_splatting_format(depth, bg, lo, hi)
            out[f"u16_{k}_{s}"] = u16
            out[f"scale_offset_{k}_{s}"] = np.array([scale, offset], np.float64)
    path = os.path.join(OUT, "depth_encode.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1_000_000
    print(f"{path}: {os.path.getsize(path)} bytes, {len(cases)} cases")


if __name__ == "__main__":
    main()
