"""Scenes of the level-1 binning tests (test_level1_model_cpu.py, test_gpu_level1.py) and the facts
about them that each case pins: superblock grid, visible rows, chunks, footprint sizes -- computed
from the oracle's `xy` / `radii` the way the rasterizer's getRect does.
"""
from __future__ import annotations

import ctypes

import numpy as np

BLOCK = 16
SB_CHUNK = 1024     # kSBChunk: level-1 chunk (doubles only past 3072 chunks, P > 3.1M)
MAX_SB = 1536       # kMaxSB
MAX_TILES_PER_SB = 256
SMALL_SB = 16       # kSmallSB: footprints over more superblocks are walked by the whole wave

CASES = [
    dict(name="one_sb_dense", P=5000, W=64, H=64, deg=1, seed=51, log_scale=-3.0),
    dict(name="chunk_1023", P=1023, W=320, H=240, deg=1, seed=52, log_scale=-3.0),
    dict(name="chunk_1024", P=1024, W=320, H=240, deg=1, seed=53, log_scale=-3.0),
    dict(name="chunk_1025", P=1025, W=320, H=240, deg=1, seed=54, log_scale=-3.0),
    dict(name="chunk_2049", P=2049, W=320, H=240, deg=1, seed=55, log_scale=-3.0),
    dict(name="culled_tail", P=6000, W=256, H=192, deg=1, seed=56, log_scale=-3.0, behind=0.6),
    dict(name="mixed_big_small", P=4000, W=640, H=480, deg=1, seed=57, log_scale=-3.5, big_frac=0.1, big_scale=20.0),
    dict(name="ties_across_chunks", P=2500, W=320, H=240, deg=1, seed=58, log_scale=-3.0, flat_z=6.0),
    dict(name="max_sb_grid", P=3000, W=2496, H=2496, deg=0, seed=59, log_scale=-2.0),
    dict(name="shift3_grid", P=3000, W=3200, H=2048, deg=0, seed=60, log_scale=-2.0),
]
IDS = [c["name"] for c in CASES]


def make_scene(c):
    from test_gpu_parity import make_scene as base_scene
    s = base_scene(c)
    if c.get("big_frac"):
        big = np.random.default_rng(c["seed"] + 7).random(c["P"]) < c["big_frac"]
        s["scales"][big] *= np.float32(c["big_scale"])
    return s


def preprocess_only(s, c):
    """The oracle's preprocess alone (what gs_oracle.forward runs first): xy, radii, depths and
    tiles_touched without sorting or rendering the frame."""
    import gs_oracle as O
    L = O.lib()
    f32, p = O._f32, O._p
    means3D = f32(s["means3D"]).reshape(-1, 3)
    P = means3D.shape[0]
    shs = f32(s["shs"])
    M = shs.reshape(P, -1, 3).shape[1]
    radii = np.zeros(P, np.int32)
    depths = np.zeros(P, np.float32)
    xy = np.zeros((P, 2), np.float32)
    conic = np.zeros((P, 4), np.float32)
    rgb = np.zeros((P, 3), np.float32)
    clamped = np.zeros((P, 3), np.uint8)
    cov3D = np.zeros((P, 6), np.float32)
    tiles = np.zeros(P, np.uint32)
    scales, rotations, opacities = f32(s["scales"]), f32(s["rotations"]), f32(s["opacities"]).reshape(P)
    view, proj, campos = f32(s["view"]).reshape(16), f32(s["proj"]).reshape(16), f32(s["campos"]).reshape(3)
    L.gso_preprocess(ctypes.c_int(P), ctypes.c_int(c["deg"]), ctypes.c_int(M), p(means3D), p(scales),
                     ctypes.c_float(1.0), p(rotations), p(opacities), p(shs), p(None),
                     p(None), p(view), p(proj), p(campos), ctypes.c_int(s["W"]), ctypes.c_int(s["H"]),
                     ctypes.c_float(np.float32(s["tanfovx"])), ctypes.c_float(np.float32(s["tanfovy"])), p(radii),
                     p(depths), p(xy), p(conic), p(rgb), p(clamped), p(cov3D), p(tiles))
    return dict(W=s["W"], H=s["H"], xy=xy, radii=radii, depths=depths, tiles_touched=tiles)


def sb_grid(W, H):
    gx, gy = (W + BLOCK - 1) // BLOCK, (H + BLOCK - 1) // BLOCK
    shift = 2
    while True:
        side = 1 << shift
        nsbx, nsby = (gx + side - 1) // side, (gy + side - 1) // side
        if nsbx * nsby <= MAX_SB or (1 << (2 * (shift + 1))) > MAX_TILES_PER_SB:
            return dict(shift=shift, nsbx=nsbx, nsby=nsby, nsb=nsbx * nsby, gx=gx, gy=gy)
        shift += 1


def depth_ordered_rects(st):
    """-> (ids, rects): the visible Gaussians in (depth bits, id) order and their tile rectangles
    (x0, y0, x1, y1 with exclusive maxima, as getRect clamps them)."""
    W, H = st["W"], st["H"]
    gx, gy = (W + BLOCK - 1) // BLOCK, (H + BLOCK - 1) // BLOCK
    r = st["radii"].astype(np.float32)
    px, py = st["xy"][:, 0].astype(np.float32), st["xy"][:, 1].astype(np.float32)
    b = np.float32(BLOCK)

    def cell(v, n):
        return np.clip(np.trunc(v / b).astype(np.int64), 0, n)
    x0, y0 = cell(px - r, gx), cell(py - r, gy)
    x1, y1 = cell(px + r + np.float32(BLOCK - 1), gx), cell(py + r + np.float32(BLOCK - 1), gy)
    n = (x1 - x0) * (y1 - y0)
    vis = (st["radii"] > 0) & (n > 0)
    np.testing.assert_array_equal(n[vis], st["tiles_touched"][vis])
    ids = np.nonzero(vis)[0]
    ids = ids[np.lexsort((ids, st["depths"].view(np.uint32)[ids]))]
    return ids, np.stack([x0, y0, x1, y1], axis=1)[ids]


def facts(st):
    g = sb_grid(st["W"], st["H"])
    ids, rects = depth_ordered_rects(st)
    sh = g["shift"]
    cover = (((rects[:, 2] - 1) >> sh) - (rects[:, 0] >> sh) + 1) * (((rects[:, 3] - 1) >> sh) - (rects[:, 1] >> sh) + 1)
    nv = len(ids)
    return dict(g, visible=nv, chunks=(nv + SB_CHUNK - 1) // SB_CHUNK, tail=nv % SB_CHUNK,
                big_rows=int((cover > SMALL_SB).sum()), max_cover=int(cover.max()) if nv else 0)


def check_facts(c, f):
    """What each case is there to cover (asserted so that a change of the scene generator cannot
    quietly move a case off its path)."""
    name, P = c["name"], c["P"]
    if name == "one_sb_dense":
        assert f["nsb"] == 1 and f["visible"] == P and f["chunks"] == 5, f
    elif name.startswith("chunk_"):
        assert f["nsb"] == 20 and f["visible"] == P, f
    elif name == "culled_tail":
        assert f["visible"] < P and 2 <= f["chunks"] <= 4 and f["tail"] != 0, f
    elif name == "mixed_big_small":
        assert f["big_rows"] >= 100 and f["max_cover"] >= 64 and f["big_rows"] < f["visible"] // 2, f
    elif name == "ties_across_chunks":
        assert f["chunks"] == 3, f
    elif name == "max_sb_grid":
        assert f["shift"] == 2 and 1400 < f["nsb"] <= MAX_SB and f["big_rows"] > 0, f
    elif name == "shift3_grid":
        assert f["shift"] == 3 and f["nsb"] == 400, f
    else:
        raise AssertionError(name)
