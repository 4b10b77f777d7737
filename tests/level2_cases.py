"""Scenes of the level-2 binning tests (test_level2_model_cpu.py, test_gpu_level2.py) and the facts
about them that each case pins: the superblock grid, the superblock lists' lengths against the
waves' LDS slots (kTBStage), which tile_bin variant the frame takes and whether its lists are cut
into slices -- computed from the oracle's preprocess the way level1_cases.py does.
"""
from __future__ import annotations

import numpy as np

import level1_cases as L1

TILE_GROUP = 16     # kTileGroup: tiles ranked per walk of a wave's batches
TB_STAGE = 7168     # kTBStage (C): list entries a workgroup holds in LDS
TB_WAVES = 8        # GSR_TB_WAVES
TB_WAVES_LONG = 16  # GSR_TB_WAVES_LONG, taken when P > TB_LONG * nsb
TB_LONG = 4096      # GSR_TB_LONG
TB_SPLIT = 16384    # GSR_TB_SPLIT: a longer list is binned in slices when the split is armed
C = TB_STAGE

ONE_SB = dict(W=64, H=64, deg=1, log_scale=-3.0)
CASES = [
    dict(name="one_sb_5", P=5, seed=70, **ONE_SB),
    dict(name="one_sb_511", P=511, seed=71, **ONE_SB),
    dict(name="one_sb_512", P=512, seed=72, **ONE_SB),
    dict(name="one_sb_513", P=513, seed=73, **ONE_SB),
    dict(name="one_sb_Cm1", P=C - 1, seed=74, **ONE_SB),
    dict(name="one_sb_C", P=C, seed=75, **ONE_SB),
    dict(name="one_sb_Cp1", P=C + 1, seed=76, **ONE_SB),
    dict(name="one_sb_2C17", P=2 * C + 17, seed=77, **ONE_SB),
    dict(name="corner_only", P=C + 232, W=256, H=192, deg=1, seed=78, log_scale=-3.5, corner=0.2),
    dict(name="ragged_200x136", P=2500, W=200, H=136, deg=1, seed=79, log_scale=-3.5, big_frac=0.08, big_scale=40.0),
    dict(name="shift3_grid", P=3000, W=3200, H=2048, deg=0, seed=60, log_scale=-2.0),
    dict(name="waves16_two_sb", P=12000, W=128, H=64, deg=0, seed=80, log_scale=-3.5),
    dict(name="split_long_list", P=TB_SPLIT + 900, seed=81, **ONE_SB),
    dict(name="ties_one_depth", P=2500, W=128, H=128, deg=1, seed=82, log_scale=-3.0, flat_z=6.0),
]
IDS = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


def make_scene(c):
    s = L1.make_scene(c)
    if c.get("corner"):
        # every mean moved along its depth plane into the frame's top-left corner
        m, f = s["means3D"], np.float32(c["corner"])
        tx, ty = np.float32(s["tanfovx"]), np.float32(s["tanfovy"])
        m[:, 0] = m[:, 0] * f - (np.float32(1) - f) * np.float32(0.95) * tx * m[:, 2]
        m[:, 1] = m[:, 1] * f - (np.float32(1) - f) * np.float32(0.95) * ty * m[:, 2]
    return s


def sb_lists(rects, g):
    """-> per superblock (row-major) the depth-ordered rows of its list and their footprints clipped
    to the superblock, as (x0, y0, x1, y1) inclusive SB-local tile coordinates."""
    sh = g["shift"]
    side = 1 << sh
    x0, y0, x1, y1 = rects[:, 0], rects[:, 1], rects[:, 2] - 1, rects[:, 3] - 1
    out = []
    for sy in range(g["nsby"]):
        for sx in range(g["nsbx"]):
            ox, oy = sx * side, sy * side
            hit = np.nonzero((x0 <= ox + side - 1) & (x1 >= ox) & (y0 <= oy + side - 1) & (y1 >= oy) & (x1 >= x0) &
                             (y1 >= y0))[0]
            loc = np.stack([np.maximum(x0[hit], ox) - ox, np.maximum(y0[hit], oy) - oy,
                            np.minimum(x1[hit], ox + side - 1) - ox, np.minimum(y1[hit], oy + side - 1) - oy], axis=1)
            out.append((hit, loc))
    return out


def tb_waves(nv, nsb):
    """tile_bin's variant: launch_binning_tiles compares the frame's Gaussian count with the grid.
    (The tests' frames cull nothing or little: the count that matters is stated per case.)"""
    return TB_WAVES_LONG if nv > TB_LONG * nsb else TB_WAVES


def facts(st, P):
    g = L1.sb_grid(st["W"], st["H"])
    ids, rects = L1.depth_ordered_rects(st)
    lists = sb_lists(rects, g)
    lens = np.array([len(h) for h, _ in lists])
    tiles = np.concatenate([(l[:, 2] - l[:, 0] + 1) * (l[:, 3] - l[:, 1] + 1) for _, l in lists]) if len(ids) else np.zeros(0)
    waves = tb_waves(P, g["nsb"])
    return dict(g, visible=len(ids), lens=lens, longest=int(lens.max()), empty_sb=int((lens == 0).sum()),
                waves=waves, slot=TB_STAGE // waves, full_sb_rows=int((tiles == 1 << (2 * g["shift"])).sum()),
                one_tile_rows=int((tiles == 1).sum()), depths=st["depths"][ids])


def check_facts(c, f):
    """What each case is there to cover."""
    name, P = c["name"], c["P"]
    seg = -(-f["longest"] // f["waves"])  # the longest wave segment of the longest list
    if name.startswith("one_sb_"):
        assert f["nsb"] == 1 and f["shift"] == 2 and f["visible"] == P and f["longest"] == P, f
        assert f["slot"] * f["waves"] == C, f
        if name == "one_sb_5":
            assert P < f["waves"] == TB_WAVES  # waves without an entry
        elif name in ("one_sb_511", "one_sb_512", "one_sb_513"):
            # 8 waves: the longest segment is a batch less one, one batch, a batch and one
            assert f["waves"] == TB_WAVES and (seg - 1) * TB_WAVES < P <= seg * TB_WAVES and seg in (64, 65), f
        elif name == "one_sb_2C17":
            assert f["waves"] == TB_WAVES_LONG and seg > 2 * f["slot"] and P < TB_SPLIT, (seg, f["slot"])  # three chunks
        else:  # C - 1, C, C + 1 (16 waves: P > TB_LONG): the longest segment fills its slot, or is one entry over
            assert f["waves"] == TB_WAVES_LONG and (seg <= f["slot"]) == (P <= C), (seg, f["slot"])
    elif name == "corner_only":
        # empty superblocks beside one whose list outgrows the 8 waves' slots
        assert f["shift"] == 2 and f["nsb"] == 12 and f["empty_sb"] >= 6 and f["waves"] == TB_WAVES, f
        assert f["lens"][0] > C and seg > f["slot"], f
    elif name == "ragged_200x136":
        assert (f["gx"], f["gy"], f["nsbx"], f["nsby"]) == (13, 9, 4, 3), f
        assert f["full_sb_rows"] >= 50 and f["one_tile_rows"] >= 500, f
    elif name == "shift3_grid":
        assert f["shift"] == 3 and f["nsb"] == 400, f
    elif name == "waves16_two_sb":
        assert f["nsb"] == 2 and P > TB_LONG * f["nsb"] and f["waves"] == TB_WAVES_LONG and f["visible"] == P, f
    elif name == "split_long_list":
        assert f["nsb"] == 1 and f["longest"] > TB_SPLIT, f
    elif name == "ties_one_depth":
        assert len(np.unique(f["depths"].view(np.uint32))) == 1 and f["nsb"] == 4, f
    else:
        raise AssertionError(name)
