"""The index arithmetic of level-1 binning's scatter (csrc/binning.hip, sb_scatter_kernel) modelled
step by step on the CPU: footprint walks without division (per lane, and wave-wide with one start
division and 64-cell skips), rounds of 512 rows, 64-bit mask words per wave and superblock, 16-bit
prefixes stored relative to the round's end, and the running position per superblock.  A wrong rank
on the device is a store outside the list, so the model asserts every position in range and written
once, and the result must equal a stable partition of the depth-ordered rows by superblock -- on the
rects of the scenes that test_gpu_level1.py renders.
"""
from __future__ import annotations

import numpy as np
import pytest

import level1_cases as L1

WAVES = 8
ROUND = 64 * WAVES


class Walk:
    """SBWalk: cell k of a footprint (row k // sw, column k % sw) stepped without division."""

    def __init__(self, foot, nsbx, k0=0):
        self.sx0, sy0, self.sw, _ = foot
        self.nsbx = nsbx
        dy = k0 // self.sw  # the one division (k0 = 0 on the per-lane walk)
        dx = k0 - dy * self.sw
        self.sx, self.sy = self.sx0 + dx, sy0 + dy
        self.key = sy0 * nsbx + self.sx0 + dy * nsbx + dx

    def next(self):
        self.sx += 1
        self.key += 1
        if self.sx == self.sx0 + self.sw:
            self.sx = self.sx0
            self.sy += 1
            self.key += self.nsbx - self.sw

    def skip(self, dy, dx):
        self.sx += dx
        self.sy += dy
        self.key += dy * self.nsbx + dx
        if self.sx >= self.sx0 + self.sw:
            self.sx -= self.sw
            self.sy += 1
            self.key += self.nsbx - self.sw


def foot_of(r, shift):
    x0, y0, x1, y1 = (int(v) for v in r)
    x1, y1 = x1 - 1, y1 - 1  # inclusive, as unpack_rect
    if x1 < x0:
        return (0, 0, 1, 0)
    sx0, sy0 = x0 >> shift, y0 >> shift
    sw = (x1 >> shift) - sx0 + 1
    return (sx0, sy0, sw, sw * ((y1 >> shift) - sy0 + 1))


def sb_local(r, sx, sy, shift):
    side = 1 << shift
    ox, oy = sx << shift, sy << shift
    x0, y0, x1, y1 = int(r[0]), int(r[1]), int(r[2]) - 1, int(r[3]) - 1
    return ((max(x0, ox) - ox) | (max(y0, oy) - oy) << 8 | (min(x1, ox + side - 1) - ox) << 16 |
            (min(y1, oy + side - 1) - oy) << 24)


def cells(foot, nsbx, lanes=None):
    """(lane, key, sx, sy) of a footprint: the per-lane walk (lanes None) or the wave-wide one."""
    n = foot[3]
    if lanes is None:
        c = Walk(foot, nsbx)
        for _ in range(n):
            yield 0, c.key, c.sx, c.sy
            c.next()
        return
    dy = 64 // foot[2]
    dx = 64 - dy * foot[2]
    for lane in range(min(64, n)):
        c = Walk(foot, nsbx, lane)
        for _ in range(lane, n, 64):
            yield lane, c.key, c.sx, c.sy
            c.skip(dy, dx)


def popcount64(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).reshape(a.shape + (64,)).sum(axis=-1).astype(np.int64)


def model(rects, g, chunk=L1.SB_CHUNK):
    """-> (base, gauss, local): the superblock bases (nsb + 1) and per list position the row and its
    clipped footprint, as sb_count / sb_colscan / sb_scatter produce them."""
    nsb, nsbx, shift = g["nsb"], g["nsbx"], g["shift"]
    nv = len(rects)
    nch = max(1, (nv + chunk - 1) // chunk)
    feet = [foot_of(r, shift) for r in rects]
    small = [f[3] <= L1.SMALL_SB for f in feet]
    # sb_count: per (SB, chunk) counts with the same walks
    cnt = np.zeros((nsb, nch), np.int64)
    for j, f in enumerate(feet):
        for _, key, sx, sy in cells(f, nsbx, None if small[j] else 64):
            assert 0 <= key < nsb and key == sy * nsbx + sx
            cnt[key, j // chunk] += 1
    col = np.cumsum(cnt, axis=1) - cnt
    tot = cnt.sum(axis=1)
    base = np.concatenate([[0], np.cumsum(tot)])
    n_entries = int(base[-1])
    gauss = np.full(n_entries, -1, np.int64)
    local = np.zeros(n_entries, np.int64)
    for c in range((nv + chunk - 1) // chunk):
        j0, j1 = c * chunk, min(nv, (c + 1) * chunk)
        run = base[:nsb] + col[:, c]
        for jr in range(j0, j1, ROUND):
            mask = np.zeros((WAVES, nsb), np.uint64)
            rows = [jr + t if jr + t < j1 else None for t in range(ROUND)]
            # 1. mark
            for t, j in enumerate(rows):
                if j is None:
                    continue
                w, lane = t >> 6, t & 63
                for _, key, _, _ in cells(feet[j], nsbx, None if small[j] else 64):
                    assert not (int(mask[w, key]) >> lane) & 1
                    mask[w, key] |= np.uint64(1 << lane)
            # 2. prefix: 16-bit, relative to the round's end
            pc = popcount64(mask)
            total = pc.sum(axis=0)
            assert total.max() <= ROUND
            pre = (((np.cumsum(pc, axis=0) - pc - total) & 0xFFFF).astype(np.uint16)).view(np.int16)
            run = run + total
            # 3. write
            for t, j in enumerate(rows):
                if j is None:
                    continue
                w, lane = t >> 6, t & 63
                below = np.uint64((1 << lane) - 1)
                for _, key, sx, sy in cells(feet[j], nsbx, None if small[j] else 64):
                    at = int(run[key]) + int(pre[w, key]) + bin(int(mask[w, key] & below)).count("1")
                    assert base[key] <= at < base[key + 1], (j, key, at)
                    assert gauss[at] < 0, "position written twice"
                    gauss[at] = j
                    local[at] = sb_local(rects[j], sx, sy, shift)
            # 4. clear: a fresh `mask` next round
        np.testing.assert_array_equal(run, base[:nsb] + col[:, c] + cnt[:, c])
    return base, gauss, local


def stable_partition(rects, g):
    """Reference: every superblock's rows in ascending depth-order slot, with the clipped footprint."""
    nsb, nsbx, shift = g["nsb"], g["nsbx"], g["shift"]
    side = 1 << shift
    x0, y0, x1, y1 = rects[:, 0], rects[:, 1], rects[:, 2] - 1, rects[:, 3] - 1
    rows, locs = [], []
    for sy in range(g["nsby"]):
        for sx in range(nsbx):
            ox, oy = sx * side, sy * side
            hit = np.nonzero((x0 <= ox + side - 1) & (x1 >= ox) & (y0 <= oy + side - 1) & (y1 >= oy) & (x1 >= x0))[0]
            rows.append(hit)
            locs.append((np.maximum(x0[hit], ox) - ox) | (np.maximum(y0[hit], oy) - oy) << 8 |
                        (np.minimum(x1[hit], ox + side - 1) - ox) << 16 | (np.minimum(y1[hit], oy + side - 1) - oy) << 24)
    counts = np.array([len(r) for r in rows])
    return np.concatenate([[0], np.cumsum(counts)]), np.concatenate(rows), np.concatenate(locs)


def check(rects, g, chunk=L1.SB_CHUNK):
    base, gauss, local = model(rects, g, chunk)
    wbase, wgauss, wlocal = stable_partition(rects, g)
    np.testing.assert_array_equal(base, wbase)
    np.testing.assert_array_equal(gauss, wgauss)
    np.testing.assert_array_equal(local, wlocal)


@pytest.mark.parametrize("c", L1.CASES, ids=L1.IDS)
def test_model_is_a_stable_partition(c):
    st = L1.preprocess_only(L1.make_scene(c), c)
    f = L1.facts(st)
    L1.check_facts(c, f)
    _, rects = L1.depth_ordered_rects(st)
    check(rects, f)


def test_model_long_chunks_and_crafted_footprints():
    """Chunks of 2048 rows (four rounds per workgroup, as large P takes them) on a crafted list: a
    full-frame footprint, single-column and single-row strips (sw = 1 and sw = nsbx: the skip's
    wrap at both ends), footprints of exactly 16 and 17 superblocks, and empty rects."""
    g = L1.sb_grid(37 * 64, 5 * 64)  # 37 x 5 superblocks of 4 x 4 tiles
    rng = np.random.default_rng(5)
    gx, gy = g["gx"], g["gy"]
    n = 4500
    x0 = rng.integers(0, gx, n)
    y0 = rng.integers(0, gy, n)
    rects = np.stack([x0, y0, np.minimum(x0 + rng.integers(1, 9, n), gx), np.minimum(y0 + rng.integers(1, 9, n), gy)], axis=1)
    crafted = [(0, 0, gx, gy), (5, 0, 6, gy), (0, 7, gx, 8), (0, 0, 64, 4), (0, 0, 68, 4), (4, 4, 36, 12),
               (3, 3, 3, 3), (0, 0, 0, 0), (gx - 1, gy - 1, gx, gy), (0, 0, 65, 8)]
    for k, r in enumerate(crafted * 6):
        rects[(k * 73 + 11) % n] = r
    check(rects.astype(np.int64), g, chunk=2048)
