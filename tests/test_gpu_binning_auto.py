"""The per-frame choice between the binning's two depth-order strategies (gsr_set_binning(2), the
default; csrc/rasterizer.hip auto_local) and the edges of the local sort's digit passes
(csrc/binning.hip sb_sort_bin_kernel).

Auto mode sends a frame through the per-superblock LDS sort only when the frame is not forwarded in
deterministic mode, its superblock grid fits one round of sb_sort_bin workgroups (two per CU) and
the list gate says the recent frames' longest superblock list fits the sort; after a frame with a
longer list the next SPLIT_MEMORY frames go straight to the global sort.  gsr_forward_stats counts
what each frame took.  Every frame compared here must equal the other path's bit for bit: the lists
are the oracle's on both.

The sort-edge cases put one 4 x 4-tile superblock's list through the local sort with list-relative
key ranges on both sides of the digit boundaries (none to four passes) and list lengths at the wave
and batch boundaries up to what the sort holds; K, keys, point list and ranges against the CPU
oracle through test_gpu_parity.compare.  The default mode now sends most frames through this sort,
which only the two-mode suites reached before.
"""
from __future__ import annotations

import contextlib

import numpy as np
import pytest

import level1_cases as L1
import level2_cases as L2
from helpers import decode_state, deterministic, rel_l2, settings, torch_inputs
from test_gpu_parity import GRAD_TOL, compare, make_scene, run_hip, run_oracle, upstream_grads

SORT_CAP = 8192     # kSortCap: the longest superblock list the local sort holds
SPLIT_MEMORY = 256  # kSplitMemory: frames a long list keeps the gates' memory

SPARSE = dict(name="sparse", P=20000, W=320, H=240, deg=3, seed=41, log_scale=-3.5)
DENSE = dict(name="dense_sb", P=60000, W=160, H=96, deg=1, seed=42, log_scale=-3.5)
TINY = dict(name="tiny_sparse", P=500, W=64, H=64, deg=1, seed=43, log_scale=-3.0)


@contextlib.contextmanager
def binning(mode):
    """gsr_set_binning(mode) for the duration; the mode found is put back."""
    from diff_gaussian_rasterization import _C
    prev = _C.set_binning(mode)
    try:
        yield prev
    finally:
        _C.set_binning(prev)


def stats():
    from diff_gaussian_rasterization import _C
    f = _C.forward_stats()
    return f["local_sort"], f["fallbacks"]


class Scene:
    """A case's tensors on the device, made once for all of its frames."""

    def __init__(self, c):
        import torch
        self.c, self.s = c, make_scene(c)
        self.dev = torch.device("cuda:0")
        self.inp = torch_inputs(self.s, self.dev, requires_grad=False)
        self.rs = settings(self.s, self.dev, c["deg"])

    def frame(self, decode=True):
        """One raw forward (no backward follows) -> (color, invdepth, radii, point list, ranges)."""
        import torch
        from diff_gaussian_rasterization import _C
        c, rs, inp = self.c, self.rs, self.inp
        e = torch.empty(0, device=self.dev)
        with torch.no_grad():
            raw = _C.rasterize_gaussians(rs.bg, inp["means3D"], e, inp["opacities"], inp["scales"], inp["rotations"],
                                         1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, c["H"], c["W"],
                                         inp["shs"], c["deg"], rs.campos, False, False, rs.render_indices,
                                         rs.parent_indices, rs.interpolation_weights, rs.num_node_kids, True)
        if not decode:
            return None
        torch.cuda.synchronize()
        st = decode_state(raw[4], raw[5], raw[6], c["P"], raw[0], c["W"], c["H"])
        return raw[1].cpu(), raw[2].cpu(), raw[3].cpu(), st["point_list"], st["ranges"]

    def fwd_bwd(self):
        import torch
        from diff_gaussian_rasterization import GaussianRasterizer
        inp = {k: v.detach().clone().requires_grad_(True) for k, v in self.inp.items()}
        color, _, invd = GaussianRasterizer(self.rs)(**inp)
        g = torch.Generator(device=self.dev).manual_seed(5)
        ((color * torch.randn(color.shape, generator=g, device=self.dev)).sum() +
         (invd * torch.randn(invd.shape, generator=g, device=self.dev)).sum()).backward()
        torch.cuda.synchronize()
        return {k: v.grad.cpu().numpy() for k, v in inp.items() if v.grad is not None}


def same_frame(a, b):
    import torch
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    np.testing.assert_array_equal(a[3], b[3])
    np.testing.assert_array_equal(a[4], b[4])


@pytest.mark.gpu
def test_auto_goes_local_with_the_same_bits():
    from diff_gaussian_rasterization import _C
    sc = Scene(SPARSE)
    with binning(1):
        want = sc.frame()
        gwant = sc.fwd_bwd()
    with binning(2):
        _C.reset_capacity_hint()
        for _ in range(3):  # the first reads K before the binning, the others defer it
            l0, f0 = stats()
            got = sc.frame()
            assert stats() == (l0 + 1, f0)
            same_frame(got, want)
        l0, f0 = stats()
        ggot = sc.fwd_bwd()
        assert stats() == (l0 + 1, f0)
    assert set(ggot) == set(gwant) and len(ggot) >= 6
    for k in gwant:
        assert rel_l2(ggot[k], gwant[k]) <= GRAD_TOL, k


@pytest.mark.gpu
def test_list_gate_after_a_fallback():
    from diff_gaussian_rasterization import _C
    sc = Scene(DENSE)
    longest = L2.facts(L1.preprocess_only(sc.s, DENSE), DENSE["P"])["longest"]
    assert longest > SORT_CAP, longest
    with binning(1):
        want = sc.frame()
    with binning(2):
        _C.reset_capacity_hint()
        l0, f0 = stats()
        same_frame(sc.frame(), want)
        assert stats() == (l0, f0 + 1)  # no history: the local sort is tried, the frame falls back
        for _ in range(3):
            same_frame(sc.frame(), want)
            assert stats() == (l0, f0 + 1)  # straight to the global sort
        _C.reset_capacity_hint()
        same_frame(sc.frame(), want)
        assert stats() == (l0, f0 + 2)
        _C.reset_capacity_hint()  # leave no long-list history behind


@pytest.mark.gpu
def test_list_gate_expires():
    import torch
    from diff_gaussian_rasterization import _C
    dense, tiny = Scene(DENSE), Scene(TINY)
    with binning(2):
        _C.reset_capacity_hint()
        l0, f0 = stats()
        dense.frame(decode=False)
        n = SPLIT_MEMORY + 44
        seen = []
        for _ in range(n):
            tiny.frame(decode=False)
            seen.append(stats()[0])
        torch.cuda.synchronize()
        l1, f1 = stats()
        _C.reset_capacity_hint()
    assert f1 == f0 + 1
    # the SPLIT_MEMORY frames after the long one stay off the local path, the other 44 are local
    # again -- but for one: a frame ends by waiting for its own K, which the global sort stores
    # before the column scan stores the list length, so the second tiny frame may still read the
    # long frame's length (the third cannot: the first tiny frame is complete by then)
    local = np.diff(np.array([l0] + seen))
    assert not local[:SPLIT_MEMORY].any(), int(local[:SPLIT_MEMORY].sum())
    assert local[-20:].all() and 43 <= l1 - l0 <= 44, (l0, l1)


@pytest.mark.gpu
def test_grid_too_large_for_one_round():
    import torch
    from diff_gaussian_rasterization import _C
    if not 576 > 2 * torch.cuda.get_device_properties(0).multi_processor_count:
        pytest.skip("576 superblocks fit one round of sb_sort_bin on this device")
    c = dict(name="street_grid", P=2000, W=1536, H=1536, deg=1, seed=44, log_scale=-3.0)
    assert L1.sb_grid(c["W"], c["H"])["nsb"] == 576
    sc = Scene(c)
    with binning(0):
        _C.reset_capacity_hint()
        l0, f0 = stats()
        want = sc.frame()
        assert stats() == (l0 + 1, f0)
    with binning(2):
        _C.reset_capacity_hint()
        l0, f0 = stats()
        got = sc.frame()
        assert stats() == (l0, f0)
    same_frame(got, want)


@pytest.mark.gpu
def test_deterministic_mode_stays_global():
    from diff_gaussian_rasterization import _C
    sc = Scene(SPARSE)
    with binning(2), deterministic():
        _C.reset_capacity_hint()
        l0, f0 = stats()
        a = sc.fwd_bwd()
        b = sc.fwd_bwd()
        assert stats() == (l0, f0)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


@pytest.mark.gpu
def test_setter_takes_three_modes():
    from diff_gaussian_rasterization import _C
    found = _C.set_binning(2)
    try:
        assert found in (0, 1, 2)
        assert _C.set_binning(0) == 2
        assert _C.set_binning(1) == 0
        assert _C.set_binning(2) == 1
        for bad in (3, -1):
            with pytest.raises(RuntimeError):
                _C.set_binning(bad)
            assert _C.set_binning(2) == 2  # a refused mode changes nothing
        assert _C._L.gsr_abi_version() == 7
    finally:
        _C.set_binning(found)


# --- the local sort's digit passes -------------------------------------------------------------

BASE = 0x3F800000  # bits(1.0f): the crafted lists' smallest key
REPEAT = 50
FAR = int(np.float32(1e8).view(np.uint32)) - BASE
EDGES = [0, 1, 255, 256, 511, 512, 513, 2 ** 18 - 1, 2 ** 18, 2 ** 18 + 1, 2 ** 27 - 1, 2 ** 27, FAR]
ONE_SB = dict(W=64, H=64, deg=1, log_scale=-3.0)


DIGIT_BITS = 8  # kSBDigitBits


def sort_passes(span):
    """LSD passes over a list whose keys span `span` = max - min: the kernel's rule."""
    return -(-int(span).bit_length() // DIGIT_BITS)


def lsd_model(keys):
    """The kernel's sort restated: stable counting passes over the digits of key - min, as many as
    the span needs -> the permutation."""
    rel = keys.astype(np.int64) - int(keys.min())
    order = np.arange(len(keys))
    for p in range(sort_passes(rel.max())):
        digit = (rel[order] >> (DIGIT_BITS * p)) & ((1 << DIGIT_BITS) - 1)
        order = order[np.argsort(digit, kind="stable")]
    return order


def test_sort_passes_of_the_edge_cases():
    """No GPU: the crafted spans sit on both sides of every pass count, and the digit split orders
    their lists as (key, id) -- ties in id order."""
    want = {0: 0, 1: 1, 255: 1, 256: 2, 511: 2, 512: 2, 513: 2, 2 ** 18 - 1: 3, 2 ** 18: 3, 2 ** 18 + 1: 3,
            2 ** 27 - 1: 4, 2 ** 27: 4, FAR: 4}
    assert {top: sort_passes(top) for top in EDGES} == want
    for bits in range(33):  # the digits cover the span, in no more than four passes
        p = sort_passes((1 << bits) - 1)
        assert p <= 4 and DIGIT_BITS * (p - 1) < bits <= DIGIT_BITS * p or bits == p == 0
    for top in EDGES:
        _, _, d = crafted_list(top, scene=False)
        keys = (np.uint32(BASE) + d.astype(np.uint32))
        np.testing.assert_array_equal(lsd_model(keys), np.lexsort((np.arange(len(keys)), keys)))


def crafted_list(top, P=3000, seed=90, scene=True):
    """One superblock (64 x 64) whose list holds every row: depth bits BASE + d, each edge d <= top on
    REPEAT scattered rows (ties must keep id order), the other rows uniform over [0, top]; every row
    in view with a footprint of a few pixels at any depth.  -> (case, scene, d)"""
    c = dict(name=f"sort_edge_{top}", P=P, seed=seed, **ONE_SB)
    rng = np.random.default_rng(seed + 1)
    d = rng.integers(0, top + 1, P, dtype=np.int64)
    edges = [e for e in EDGES if e <= top]
    rows = rng.permutation(P)[:REPEAT * len(edges)].reshape(len(edges), REPEAT)
    for e, r in zip(edges, rows):
        d[r] = e
    if not scene:
        return c, None, d
    s = make_scene(c)
    z = (np.uint32(BASE) + d.astype(np.uint32)).view(np.float32)
    m = s["means3D"]
    m[:, 0] = z * rng.uniform(-0.6, 0.6, P).astype(np.float32) * np.float32(s["tanfovx"])
    m[:, 1] = z * rng.uniform(-0.6, 0.6, P).astype(np.float32) * np.float32(s["tanfovy"])
    m[:, 2] = z
    s["scales"][:] = (np.float32(0.02) * z)[:, None]
    return c, s, d


def run_local(c, s):
    """A frame pair (run_hip) through the local sort, against the oracle; both frames sorted in LDS."""
    dcol, dinv = upstream_grads(c)
    st, g = run_oracle(s, c, dcol, dinv)
    f = L2.facts(L1.preprocess_only(s, c), c["P"])
    assert f["nsb"] == 1 and f["visible"] == c["P"] and f["longest"] == c["P"] <= SORT_CAP, f
    with binning(0):
        l0, f0 = stats()
        h = run_hip(s, c, dcol, dinv)
        assert stats() == (l0 + 2, f0)
    compare(c, st, g, h, check_grads=False)
    return h


@pytest.mark.gpu
@pytest.mark.parametrize("top", EDGES[1:], ids=[f"span_{t}" for t in EDGES[1:]])
def test_sort_digit_edges(top):
    c, s, d = crafted_list(top)
    assert d.min() == 0 and d.max() == top
    h = run_local(c, s)
    np.testing.assert_array_equal(h["state"]["depths"].view(np.uint32), np.uint32(BASE) + d.astype(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513, 8191, 8192])
def test_sort_list_lengths(n):
    c = dict(name=f"sort_len_{n}", P=n, seed=100 + n % 97, **ONE_SB)
    run_local(c, L2.make_scene(c))


@pytest.mark.gpu
def test_sort_all_depths_equal():
    c = dict(name="sort_one_depth", P=2500, seed=83, flat_z=6.0, **ONE_SB)
    s = L2.make_scene(c)
    assert len(np.unique(s["means3D"][:, 2].view(np.uint32))) == 1
    run_local(c, s)
