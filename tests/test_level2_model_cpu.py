"""Level-2 binning (csrc/binning.hip: tb_rank, tb_walk_s, tb_bases, tb_split_kernel) modelled on the
CPU: a batch's row and column masks and their AND per tile, the waves' contiguous segments walked
through an LDS slot of kTBStage / waves entries in chunks, the per-wave tile counts, the tile bases
in SB-local row-major order with waves in list order, and the slices of a split list.

* The AND of row and column masks must equal, bit for bit, what the kernel it replaces computed
  per tile (`group_mask`, restated here), for every tile group: over every SB-clipped rectangle at
  shifts 2 and 3, over all rectangles touching an edge plus a seeded sample at shift 4, and for
  the padding word at every shift -- also through the 4-bit packing the local sort stores.
* A wrong rank on the device is a store outside the list, so the model asserts every position
  written once and inside its tile's range, and the result must be the stable partition of each
  superblock's list by tile -- on the rects of the scenes that test_gpu_level2.py renders.
"""
from __future__ import annotations

import numpy as np
import pytest

import level1_cases as L1
import level2_cases as L2

PAD = 0xFF
U32 = 0xFFFFFFFF


def pack8(x0, y0, x1, y1):
    return x0 | y0 << 8 | x1 << 16 | y1 << 24


def group_mask(r, tg, shift):
    """The replaced kernel's per-lane footprint over tile group [tg, tg + 16): one bit per tile."""
    r = np.asarray(r, np.int64)
    side = 1 << shift
    x0, y0, x1, y1 = r & 0xFF, (r >> 8) & 0xFF, (r >> 16) & 0xFF, r >> 24
    cols = ((2 << np.minimum(x1, 31)) - 1) & ~((1 << np.minimum(x0, 31)) - 1)
    row0, rows = tg >> shift, L2.TILE_GROUP >> shift
    m = np.zeros_like(r)
    for q in range(rows):
        ry = row0 + q
        m |= np.where((ry >= y0) & (ry <= y1), (cols << (q * side)) & U32, 0)
    return np.where(x1 < x0, 0, m)


def foot(x0, y0, x1, y1):
    """tb_foot: first column / row and the clamped numbers of columns / rows."""
    return x0, y0, np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)


def foot8(r):
    r = np.asarray(r, np.int64)
    return foot(r & 0xFF, (r >> 8) & 0xFF, (r >> 16) & 0xFF, r >> 24)


def pack4(r):
    r = np.asarray(r, np.int64)
    return (r & 0xF) | ((r >> 4) & 0xF0) | ((r >> 8) & 0xF00) | ((r >> 12) & 0xF000)


def foot4(h):
    return foot(h & 0xF, (h >> 4) & 0xF, (h >> 8) & 0xF, (h >> 12) & 0xF)


def row_col_masks(f, tg, shift):
    """tb_rank's lane predicates: unsigned (c - x0) < nx per column of the group, (row - y0) < ny
    per row.  -> (rows [R, n], cols [C, n]) booleans per entry."""
    x0, y0, nx, ny = f
    ncols, nrows = 1 << shift, L2.TILE_GROUP >> shift
    row0 = tg >> shift
    cols = np.stack([((c - x0) & U32) < nx for c in range(ncols)])
    rows = np.stack([((row0 + q - y0) & U32) < ny for q in range(nrows)])
    return rows, cols


def and_mask(f, tg, shift):
    """The 16 tile predicates of a group as group_mask lays its bits out."""
    rows, cols = row_col_masks(f, tg, shift)
    m = np.zeros(rows.shape[1], np.int64)
    for k in range(L2.TILE_GROUP):
        m |= (rows[k >> shift] & cols[k & ((1 << shift) - 1)]).astype(np.int64) << k
    return m


def clipped_rects(shift, edge_only=False):
    side = 1 << shift
    a = np.arange(side)
    x0, x1, y0, y1 = (v.ravel() for v in np.meshgrid(a, a, a, a, indexing="ij"))
    ok = (x0 <= x1) & (y0 <= y1)
    if edge_only:
        ok &= (x0 == 0) | (y0 == 0) | (x1 == side - 1) | (y1 == side - 1)
    return pack8(x0[ok], y0[ok], x1[ok], y1[ok])


def check_identity(r, shift):
    for tg in range(0, 1 << (2 * shift), L2.TILE_GROUP):
        want = group_mask(r, tg, shift)
        np.testing.assert_array_equal(and_mask(foot8(r), tg, shift), want)
        np.testing.assert_array_equal(and_mask(foot4(pack4(r)), tg, shift), want)


@pytest.mark.parametrize("shift", [2, 3])
def test_mask_identity_every_clipped_rect(shift):
    r = clipped_rects(shift)
    side = 1 << shift
    assert len(r) == (side * (side + 1) // 2) ** 2
    check_identity(r, shift)


def test_mask_identity_shift4_edges_and_sample():
    edge = clipped_rects(4, edge_only=True)
    every = clipped_rects(4)
    sample = every[np.random.default_rng(4).choice(len(every), 3000, replace=False)]
    assert len(edge) > 4000
    check_identity(np.concatenate([edge, sample]), 4)


@pytest.mark.parametrize("shift", [2, 3, 4])
def test_padding_word_has_no_tiles(shift):
    pad = np.array([PAD], np.int64)
    assert foot4(pack4(pad))[2][0] == 0 and foot8(pad)[2][0] == 0
    for tg in range(0, 1 << (2 * shift), L2.TILE_GROUP):
        assert group_mask(pad, tg, shift)[0] == 0
        assert and_mask(foot8(pad), tg, shift)[0] == 0
        assert and_mask(foot4(pack4(pad)), tg, shift)[0] == 0


# ---------------------------------------------------------------------------------------------


def walk(loc8, ids, a, b, waves, shift, tc, place, out=None, lo=None, hi=None, seen=None):
    """tb_walk_s over entries [a, b) of one list: count (tc[w][t] = the wave's tile counts) or place
    (from the wave's tile starts tc[w][t]).  A segment longer than the slot goes through it in
    chunks, tc[w][] carrying the tiles' counts / positions between chunks."""
    slot = L2.TB_STAGE // waves
    assert slot % 64 == 0 and slot * waves == L2.TB_STAGE
    tps = 1 << (2 * shift)
    n = b - a
    for w in range(waves):
        seg0, seg1 = a + n * w // waves, a + n * (w + 1) // waves
        fits = seg1 - seg0 <= slot
        if not place and seg0 == seg1:
            tc[w, :tps] = 0
        for c0 in range(seg0, seg1, slot):
            c1 = min(seg1, c0 + slot)
            nb = (c1 - c0 + 63) >> 6
            assert nb <= slot // 64
            # the slot as staged: the chunk's entries, the last batch padded
            stage_r = np.full(nb * 64, PAD, np.int64)
            stage_i = np.zeros(nb * 64, np.int64)
            stage_r[:c1 - c0] = loc8[c0:c1]
            stage_i[:c1 - c0] = ids[c0:c1]
            first = c0 == seg0
            for tg in range(0, tps, L2.TILE_GROUP):
                acc = tc[w, tg:tg + L2.TILE_GROUP].copy() if (place or not first) else np.zeros(L2.TILE_GROUP, np.int64)
                for d in range(nb):
                    r, gid = stage_r[d * 64:(d + 1) * 64], stage_i[d * 64:(d + 1) * 64]
                    rows, cols = row_col_masks(foot4(pack4(r)), tg, shift)  # the slot holds 4-bit fields
                    for k in range(L2.TILE_GROUP):
                        bm = rows[k >> shift] & cols[k & ((1 << shift) - 1)]  # the tile's lanes
                        cnt = int(bm.sum())
                        if place and cnt:
                            at = acc[k] + np.cumsum(bm)[bm] - 1  # base + lanes below in the mask
                            t = tg + k
                            assert lo[t] <= at.min() and at.max() < hi[t], (w, t, at, lo[t], hi[t])
                            assert not seen[at].any(), "position written twice"
                            seen[at] = True
                            out[at] = gid[bm]
                        acc[k] += cnt
                if not place or not fits:
                    tc[w, tg:tg + L2.TILE_GROUP] = acc


def bases(tc, waves, tps, base, tot=None, extra=None):
    """tb_bases: tiles in SB-local row-major order from `base`, waves in list order.
    -> (lo, hi) of every tile's range; tc becomes the waves' starts."""
    c = tc[:waves, :tps].sum(axis=0) if tot is None else tot
    lo = base + np.cumsum(c) - c
    b = lo + (extra if extra is not None else 0)
    for k in range(waves):
        ck = tc[k, :tps].copy()
        tc[k, :tps] = b
        b = b + ck
    return lo, lo + c


def tile_bin(loc8, ids, shift, waves, base, out, seen):
    tps = 1 << (2 * shift)
    tc = np.full((waves, L1.MAX_TILES_PER_SB), -1, np.int64)
    walk(loc8, ids, 0, len(ids), waves, shift, tc, place=False)
    assert (tc[:, :tps] >= 0).all(), "a wave left a tile count unset"
    lo, hi = bases(tc, waves, tps, base)
    walk(loc8, ids, 0, len(ids), waves, shift, tc, place=True, out=out, lo=lo, hi=hi, seen=seen)
    return lo, hi


def tb_split(loc8, ids, shift, base, out, seen, nsl):
    """tb_split_kernel's two launches over the list's nsl slices (16 waves each)."""
    waves, tps, L = L2.TB_WAVES_LONG, 1 << (2 * shift), len(ids)
    Ls = (L + nsl - 1) // nsl
    cuts = [(min(L, j * Ls), min(L, min(L, j * Ls) + Ls)) for j in range(nsl)]
    cnt = np.zeros((nsl, tps), np.int64)
    for j, (a, b) in enumerate(cuts):
        tc = np.full((waves, L1.MAX_TILES_PER_SB), -1, np.int64)
        walk(loc8, ids, a, b, waves, shift, tc, place=False)
        cnt[j] = tc[:, :tps].sum(axis=0)
    tot = cnt.sum(axis=0)
    for j, (a, b) in enumerate(cuts):
        tc = np.full((waves, L1.MAX_TILES_PER_SB), -1, np.int64)
        walk(loc8, ids, a, b, waves, shift, tc, place=False)
        lo, hi = bases(tc, waves, tps, base, tot=tot, extra=cnt[:j].sum(axis=0))
        walk(loc8, ids, a, b, waves, shift, tc, place=True, out=out, lo=lo, hi=hi, seen=seen)
    return lo, hi


def stable_by_tile(hit, loc, shift):
    """Reference: per tile of the SB (row-major), the list's rows covering it, in list order."""
    side = 1 << shift
    rows, counts = [], []
    for t in range(side * side):
        x, y = t & (side - 1), t >> shift
        m = (loc[:, 0] <= x) & (x <= loc[:, 2]) & (loc[:, 1] <= y) & (y <= loc[:, 3])
        rows.append(hit[m])
        counts.append(int(m.sum()))
    return np.concatenate(rows) if rows else np.zeros(0, np.int64), np.array(counts)


def check_frame(rects, f, split=False):
    shift = f["shift"]
    lists = L2.sb_lists(rects, f)
    K = int(sum(((l[:, 2] - l[:, 0] + 1) * (l[:, 3] - l[:, 1] + 1)).sum() for _, l in lists))
    out = np.full(K, -1, np.int64)
    seen = np.zeros(K, bool)
    base = 0
    for hit, loc in lists:
        loc8 = pack8(loc[:, 0], loc[:, 1], loc[:, 2], loc[:, 3])
        want, counts = stable_by_tile(hit, loc, shift)
        if split and len(hit) > L2.TB_SPLIT:
            nsl = min((len(hit) + L2.TB_SPLIT - 1) // L2.TB_SPLIT, 63)
            assert nsl >= 2
            lo, hi = tb_split(loc8, hit, shift, base, out, seen, nsl)
        else:
            lo, hi = tile_bin(loc8, hit, shift, f["waves"], base, out, seen)
        np.testing.assert_array_equal(hi - lo, counts)
        np.testing.assert_array_equal(out[base:base + len(want)], want)
        base += len(want)
    assert base == K and seen.all()


@pytest.mark.parametrize("c", L2.CASES, ids=L2.IDS)
def test_model_is_a_stable_partition_by_tile(c):
    st = L1.preprocess_only(L2.make_scene(c), c)
    f = L2.facts(st, c["P"])
    L2.check_facts(c, f)
    _, rects = L1.depth_ordered_rects(st)
    check_frame(rects, f)
    if c["name"] == "split_long_list":
        check_frame(rects, f, split=True)


def test_model_shift4_crafted_lists():
    """A 16 x 16-tile superblock (16 tile groups of one row each), which the device tests reach only
    above 25 Mpix: full-SB, single-row, single-column and single-tile footprints among random
    ones, with 8 and with 16 waves, the second with segments over several slot chunks."""
    rng = np.random.default_rng(44)
    for waves, n in ((8, 700), (L2.TB_WAVES_LONG, L2.TB_STAGE + 300)):
        x0, y0 = rng.integers(0, 16, n), rng.integers(0, 16, n)
        x1 = np.minimum(x0 + rng.integers(0, 5, n), 15)
        y1 = np.minimum(y0 + rng.integers(0, 5, n), 15)
        loc = np.stack([x0, y0, x1, y1], axis=1)
        crafted = [(0, 0, 15, 15), (0, 7, 15, 7), (9, 0, 9, 15), (15, 15, 15, 15), (0, 0, 0, 0), (0, 15, 15, 15)]
        for k, r in enumerate(crafted * 5):
            loc[(k * 37 + 5) % n] = r
        hit = np.arange(n) * 3 + 1
        K = int(((loc[:, 2] - loc[:, 0] + 1) * (loc[:, 3] - loc[:, 1] + 1)).sum())
        out, seen = np.full(K, -1, np.int64), np.zeros(K, bool)
        lo, hi = tile_bin(pack8(*loc.T), hit, 4, waves, 0, out, seen)
        want, counts = stable_by_tile(hit, loc, 4)
        np.testing.assert_array_equal(hi - lo, counts)
        np.testing.assert_array_equal(out, want)
        assert seen.all()
