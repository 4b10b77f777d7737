"""The depth sort's 9-bit digits over near-plane-relative keys (csrc/dsort.hip): a frame whose visible
depth bits lie in [base, base + 2^27), base = bits(0.2f), is ordered by three passes (pass 2 writes the
order, pass 3 returns at once); any other frame takes the fourth pass, decided on the device.  Every
frame queues its four pass launches: the host hint that queues three and completes a wide frame by a
late pass is not part of this build, so where a late-pass frame would be expected the tests assert the
four-launch behaviour instead (sort_wide_frames counts the frame, sort_late_pass stays put).

Crafted depths are set from bit patterns; the crafted rows sit near the optical axis with a scale
that grows with depth (bounded so that its square stays finite), and every one of them is asserted
to be on screen.  Order, binning, image and gradients are compared with the CPU oracle at the bars
of test_gpu_parity.py.  At z = 3e38 the oracle's own position gradient is NaN (z * z overflows
fp32 in its derivative, wherever the row is put), so there is no reference value for those rows: the
rows whose oracle gradient is not finite must all be 3e38 rows, and they are left out of that one
comparison; every other row and every other tensor is compared in full.  The ticket path (more tiles than resident workgroups) is covered by that
file's 3M-row tests.
"""
from __future__ import annotations

import numpy as np
import pytest

from test_gpu_parity import binning_mode, compare, make_scene, run_hip, run_oracle, upstream_grads

BASE = 0x3E4CCCCD  # bits(0.2f): the preprocess's near plane
REPEAT = 50


def f32(bits):
    return np.uint32(bits).view(np.float32)


NARROW_BITS = [BASE + d for d in (1, 2, 511, 512, 513, 2 ** 18 - 1, 2 ** 18, 2 ** 18 + 1, 2 ** 27 - 1)]
WIDE_BITS = [BASE + 2 ** 27 - 1, BASE + 2 ** 27] + [int(np.float32(z).view(np.uint32)) for z in (1e5, 1e8, 3e38)]


def crafted_scene(bits, P=20000, W=128, H=96, seed=30, name="dsort3"):
    """20 000 rows on screen with depths U[2, 10] (as test_sort_tile_boundaries_with_culled_rows builds
    them), and each pattern of `bits` as the depth of REPEAT scattered rows -> (case, scene, rows)."""
    c = dict(name=name, P=P, W=W, H=H, deg=1, seed=seed, log_scale=-3.5)
    s = make_scene(c)
    rng = np.random.default_rng(seed + 1)
    m = s["means3D"]
    z = rng.uniform(2.0, 10.0, P).astype(np.float32)
    ux = rng.uniform(-0.6, 0.6, P).astype(np.float32)
    uy = rng.uniform(-0.6, 0.6, P).astype(np.float32)
    rows = rng.permutation(P)[:REPEAT * len(bits)].reshape(len(bits), REPEAT)
    for b, r in zip(bits, rows):
        z[r] = f32(b)
        # near the axis (x * focal must stay finite at 3e38), a footprint of a few pixels at any depth
        ux[r] *= np.float32(1e-4)
        uy[r] *= np.float32(1e-4)
        s["scales"][r] = np.minimum(np.float32(0.02) * z[r], np.float32(1e15))[:, None]
    m[:, 0] = z * ux * np.float32(s["tanfovx"])
    m[:, 1] = z * uy * np.float32(s["tanfovy"])
    m[:, 2] = z
    return c, s, rows.reshape(-1)


def run_case(c, s, rows, oracle=None):
    """One frame pair through the global sort (run_hip: a raw call, then the autograd path) against the
    oracle; the crafted rows on screen with their exact depth bits; the order as
    test_depth_order_large checks it."""
    dcol, dinv = upstream_grads(c)
    st, g = oracle if oracle is not None else run_oracle(s, c, dcol, dinv)
    with binning_mode(1):
        h = run_hip(s, c, dcol, dinv)
    S = h["state"]
    assert np.all(h["radii"][rows] > 0) and np.all(S["tiles_touched"][rows] > 0)
    dbits = S["depths"].view(np.uint32)
    np.testing.assert_array_equal(dbits[rows], s["means3D"][rows, 2].view(np.uint32))
    vis = (h["radii"] > 0) & (S["tiles_touched"] > 0)
    ids = np.nonzero(vis)[0]
    np.testing.assert_array_equal(S["order"][:len(ids)], ids[np.lexsort((ids, dbits[ids]))])
    # rows without a reference gradient (module docstring): only position gradients of 3e38 rows
    P = c["P"]
    no_ref = np.zeros(P, bool)
    for k, v in g.items():
        if k.startswith("dL_d") and v.size % P == 0 and v.size:
            bad = ~np.isfinite(np.asarray(v).reshape(P, -1)).all(axis=1)
            assert k == "dL_dmeans3D" or not bad.any(), k
            no_ref |= bad
    assert np.all(s["means3D"][no_ref, 2] > np.float32(1e38))
    if no_ref.any():
        g = dict(g, dL_dmeans3D=np.where(no_ref[:, None], 0.0, g["dL_dmeans3D"].reshape(P, 3)).astype(np.float32))
        h["grads"]["means3D"] = np.where(no_ref[:, None], 0.0, h["grads"]["means3D"].reshape(P, 3)).astype(np.float32)
    compare(c, st, g, h, global_sort=True)
    return st, g


def sort_stats():
    from diff_gaussian_rasterization import _C
    f = _C.forward_stats()
    return f["sort_wide_frames"], f["sort_late_pass"]


@pytest.fixture(scope="module")
def narrow():
    c, s, rows = crafted_scene(NARROW_BITS, name="dsort3_digit_edges")
    return c, s, rows, run_oracle(s, c, *upstream_grads(c))


@pytest.fixture(scope="module")
def wide():
    c, s, rows = crafted_scene(WIDE_BITS, name="dsort3_window_edge")
    return c, s, rows, run_oracle(s, c, *upstream_grads(c))


@pytest.mark.gpu
def test_digit_and_tie_edges(narrow):
    """Depth bits at the digit boundaries of base + d (d = 1, 2, 511, 512, 513, 2^18 - 1, 2^18,
    2^18 + 1, 2^27 - 1), each on 50 scattered rows (ties keep id order): a narrow frame, exact."""
    c, s, rows, oracle = narrow
    w0, l0 = sort_stats()
    run_case(c, s, rows, oracle)
    assert sort_stats() == (w0, l0)


@pytest.mark.gpu
def test_window_edge_and_beyond(narrow, wide):
    """Rows at base + 2^27 - 1 (13107.199, inside the window) and base + 2^27 (13107.2, outside), 1e5,
    1e8 and 3e38: the fourth pass orders the frame.  Three frame pairs after a capacity reset (the
    first frame reads K before the binning, the others defer it): wide, wide again, narrow -- each
    exact; the wide frames are counted, the narrow ones are not, and no frame needs a late pass."""
    from diff_gaussian_rasterization import _C
    c, s, rows, oracle = wide
    _C.reset_capacity_hint()
    w0, l0 = sort_stats()
    run_case(c, s, rows, oracle)
    assert sort_stats() == (w0 + 2, l0)  # run_hip runs two frames
    run_case(c, s, rows, oracle)
    assert sort_stats() == (w0 + 4, l0)
    cn, sn, rn, on = narrow
    run_case(cn, sn, rn, on)
    assert sort_stats() == (w0 + 4, l0)


@pytest.mark.gpu
def test_wide_frame_with_deferred_K(narrow, wide):
    """A narrow frame leaves a capacity hint, so the wide frame after it is queued whole -- sort,
    binning and render -- before the host has read K or `wide`: exact all the same, and the narrow
    frame after it runs without a sticky error from the wide one."""
    cn, sn, rn, on = narrow
    c, s, rows, oracle = wide
    run_case(cn, sn, rn, on)
    w0, l0 = sort_stats()
    run_case(c, s, rows, oracle)
    assert sort_stats() == (w0 + 2, l0)
    run_case(cn, sn, rn, on)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [NARROW_BITS, WIDE_BITS], ids=["narrow", "wide"])
def test_no_rect_carry(bits):
    """A frame more than 255 tiles wide (4112 x 16, P = 2000): no 4-B rects, so nothing is carried
    through the passes and the last pass -- pass 2 when narrow, pass 3 when wide -- gathers the 8-B
    rects."""
    c, s, rows = crafted_scene(bits, P=2000, W=4112, H=16, seed=33, name="dsort3_rect8")
    w0, l0 = sort_stats()
    run_case(c, s, rows)
    assert sort_stats() == (w0 + (2 if bits is WIDE_BITS else 0), l0)
