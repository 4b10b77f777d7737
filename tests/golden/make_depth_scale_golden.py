"""Generate tests/golden/depth_scale.npz from the reference's own get_scales (build container only).

preprocess/make_depth_scale.py's get_scales is imported from the reference and run on a handful of small
images, with a stub cv2 module: imread returns the image's map (or None: no file) and remap is this
project's statement of the bilinear sample (tests/depth_scale_ref.py sample), returned with shape (n, 1)
as OpenCV returns it.  OpenCV itself cannot be run here, so the sample is restated and everything around
it -- the point mask, the transform, the validity tests, the acceptance, numpy's medians and means, the
scale and offset -- is the reference's.  get_scales reads the module global images_metas, which its
__main__ block sets; it is set here.

Stored: point_id, point_xyz (shared), n; per image k: q_k, t_k, wh_k (width, height), xy_k, pid_k,
u16_k (absent when has_map_k is 0), has_map_k, and ref_k = (scale, offset) as get_scales returned them.
general_k is 1 for the image with a general rotation: there the reference's np.dot goes through the BLAS,
whose kernels fuse the products of the transform on some machines and not on others (and not for every
size), so its outputs are this machine's; every other image has a rotation of entries 0, +-1 and points
on a 2^-8 grid, which makes the transform exact up to its last addition on any machine.

Nothing from the reference is copied; only numbers are kept.
Usage:  python tests/golden/make_depth_scale_golden.py --ref <reference checkout>
"""
from __future__ import annotations

import argparse
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import depth_scale_ref as R  # noqa: E402


def quat(rng, angle):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * ax])


def images(rng):
    """The point table and the images: (q, t, width, height, xy, pid, u16 or None)."""
    N = 400
    point_id = rng.permutation(600)[:N].astype(np.int64)  # ids 0 .. 599 with gaps
    # coordinates on a 2^-8 grid: with a rotation of entries 0, +-1 every product and sum of the transform
    # is exact however a BLAS orders or fuses them, and only the + t rounds
    point_xyz = np.round(np.stack([rng.uniform(-8, 8, N), rng.uniform(-5, 5, N), rng.uniform(3, 40, N)], 1) * 256) / 256
    have = point_id.copy()
    gaps = np.setdiff1d(np.arange(int(point_id.max())), point_id)

    def view(n, width, height, Hd, Wd, q=(1.0, 0.0, 0.0, 0.0), ids=None, smooth=True):
        q, t = np.asarray(q, np.float64), rng.normal(size=3) * 0.3
        xy = np.stack([rng.uniform(0, width, n), rng.uniform(0, height, n)], 1)
        pid = rng.choice(have, n) if ids is None else ids
        yy, xx = np.mgrid[0:Hd, 0:Wd]
        u16 = (9000 + 40000 * (xx / Wd) * (yy / Hd) + rng.integers(0, 2000, (Hd, Wd))).astype(np.uint16) if smooth \
            else rng.integers(0, 65536, (Hd, Wd)).astype(np.uint16)
        return [q, t, width, height, xy, pid.astype(np.int64), u16]

    out = []
    out.append(view(40, 64, 48, 24, 32))                                    # s = 1 / 2, even count
    v = view(57, 96, 64, 64, 96, smooth=False)                              # s = 1: ids in gaps, >= T, -1, outside
    v[5][:6] = [gaps[0], gaps[1], 600, 10 ** 9, -1, -1]
    v[4][6], v[4][7], v[4][8] = [-0.25, 3.0], [96.0, 3.0], [5.0, 64.0]
    out.append(v)
    out.append(view(10, 64, 48, 48, 64))                                    # 10 valid: not fitted
    out.append(view(11, 64, 48, 48, 64))                                    # 11 valid: fitted
    v = view(30, 64, 48, 24, 32, ids=np.full(30, have[3]))                  # one point 30 times: range 0
    out.append(v)
    v = view(33, 64, 48, 24, 32)                                            # a flat map: s_mono = 0, inf / -inf
    v[6][:] = 12345
    out.append(v)
    v = view(16, 64, 48, 48, 64)                                            # 16 valid at whole pixels of a coarse map:
    v[4] = np.stack([rng.integers(0, 63, 16), rng.integers(0, 47, 16)], 1).astype(np.float64)  # every sum exact in fp32
    v[6] = (rng.integers(0, 256, (48, 64)) * 256).astype(np.uint16)
    out.append(v)
    out.append(view(257, 48, 32, 64, 96, q=(0.0, 0.0, 0.0, 1.0)))           # s = 2, odd count, half a turn about z
    out.append(view(45, 96, 64, 21, 32, q=(0.5, 0.5, 0.5, 0.5)))            # s = 21 / 64; z = Y + t2: half behind
    out.append(view(25, 64, 48, 24, 32, q=(0.0, 1.0, 0.0, 0.0)))            # turned round: every point behind
    out.append(view(90, 64, 48, 24, 32, q=quat(rng, 0.4)))                  # a general rotation (general_k = 1)
    v = view(20, 64, 48, 24, 32)                                            # no map
    v[6] = None
    out.append(v)
    return point_id, point_xyz, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout")
    a = ap.parse_args()
    store = {}
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_UNCHANGED, cv2.INTER_LINEAR, cv2.BORDER_REPLICATE = -1, 1, 1
    cv2.imread = lambda path, flag=None: store.get(os.path.basename(path))
    cv2.remap = lambda src, mx, my, interpolation=None, borderMode=None: R.sample(src, mx, my)[:, None]
    sys.modules["cv2"] = cv2
    sys.path.insert(0, os.path.join(a.ref, "preprocess"))
    import make_depth_scale as ref

    rng = np.random.default_rng(24)
    point_id, point_xyz, imgs = images(rng)
    ordered = np.zeros([point_id.max() + 1, 3])
    ordered[point_id] = point_xyz
    out = dict(point_id=point_id, point_xyz=point_xyz, n=np.int64(len(imgs)))
    cams, metas = {}, {}
    for k, (q, t, width, height, xy, pid, u16) in enumerate(imgs):
        cams[k] = types.SimpleNamespace(width=width, height=height)
        metas[k] = types.SimpleNamespace(camera_id=k, qvec=q, tvec=t, xys=xy, point3D_ids=pid, name=f"im{k}.jpg")
        if u16 is not None:
            store[f"im{k}.png"] = u16
    ref.images_metas = metas
    args = types.SimpleNamespace(depths_dir="depths")
    for k, (q, t, width, height, xy, pid, u16) in enumerate(imgs):
        with np.errstate(all="ignore"):
            got = ref.get_scales(k, cams, metas, ordered, args)
        out[f"q_{k}"], out[f"t_{k}"], out[f"wh_{k}"] = q, t, np.array([width, height], np.int64)
        out[f"xy_{k}"], out[f"pid_{k}"] = xy, pid
        out[f"has_map_{k}"] = np.int64(u16 is not None)
        out[f"general_{k}"] = np.int64(bool(np.any((np.abs(q) != 0) & (np.abs(q) != 0.5) & (np.abs(q) != 1))))
        if u16 is None:
            assert got is None
            out[f"ref_{k}"] = np.zeros(2)
            continue
        out[f"u16_{k}"] = u16
        assert got["image_name"] == f"im{k}"
        out[f"ref_{k}"] = np.array([got["scale"], got["offset"]], np.float64)
        print(k, len(pid), got["scale"], got["offset"])
    path = os.path.join(OUT, "depth_scale.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
