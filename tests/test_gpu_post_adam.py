"""gsr_post_adam_step alone (include/gsr_post.h, csrc/post_step.hip): the locked rows' zeroing, the
dense Adam and the gradients' clear over persistent gradients, against the path it replaces run on
copies (tests/post_adam_cases.py).  Parameters, both moments and `live` bit for bit; the gradient
buffers all zero bits after every step.

Mutation check (profiles/r27_post_mutation_check.txt): scratch builds from mutated copies of the
sources, loaded through GSR_LIBRARY -- an updated row's gradient not cleared; idle live rows skipped;
gsr_cut_mark_rows omitting the parents -- each fail tests of this file and of test_gpu_post_stage.py.
"""
from __future__ import annotations

import pytest
import torch

import post_adam_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _lock_bytes(N, anchors):
    if anchors.numel() == 0:
        return None
    lock = torch.zeros(N, dtype=torch.uint8, device=DEV)
    lock[anchors] = 1
    return lock


def _assert_same(tag, got, want):
    for name, a, b in zip(("xyz", "features", "opacity", "scaling", "rotation"), got, want):
        assert torch.equal(C.bits(a), C.bits(b)), (tag, name, int((C.bits(a) != C.bits(b)).sum()))


@pytest.mark.parametrize("N", C.ROWS)
def test_post_adam_matches_zero_rows_then_dense_adam(N):
    for ci, (tkind, tail, akind, mkind) in enumerate(C.combos(N)):
        tag = (N, tkind, tail, akind, mkind)
        g = torch.Generator(device=DEV).manual_seed(1000 * ci + N)
        touched = C.touched_rows(tkind, N, DEV)
        anchors = C.anchor_rows(akind, N, touched, g, DEV)
        P, M, V, G = C.make_state(N, mkind, touched, g, DEV)
        rP, rM, rV, rG = ([t.clone() for t in ts] for ts in (P, M, V, G))
        P0 = [t.clone() for t in P]
        C.reference_step(rP, rG, rM, rV, tail, anchors, step=3)

        live = C.live_build(M, V, DEV)
        nonzero = torch.zeros(N, dtype=torch.bool, device=DEV)
        for t in M + V:
            nonzero |= (C.bits(t) != 0).any(1)
        assert torch.equal(live, nonzero.to(torch.uint8)), tag  # -0.0 and denormals count
        stamp = torch.zeros(N, dtype=torch.int32, device=DEV)
        stamp[touched] = 5
        stamp[~(stamp == 5)] = 4  # an older iteration's value is not this one's
        locked = torch.zeros(N, dtype=torch.bool, device=DEV)
        locked[N - tail:] = True
        locked[anchors] = True
        is_touched = stamp == 5
        want_live = live | (is_touched & ~locked).to(torch.uint8)
        C.post_step(P, G, M, V, stamp, 5, live, tail, _lock_bytes(N, anchors), step=3)
        _assert_same(tag + ("param",), P, rP)
        _assert_same(tag + ("exp_avg",), M, rM)
        _assert_same(tag + ("exp_avg_sq",), V, rV)
        assert torch.equal(live, want_live), tag
        for t in G:
            assert int((C.bits(t) != 0).sum()) == 0, tag  # every gradient is zero bits on return
        # a row that never was live holds +0 moments
        dead = live == 0
        for t in M + V:
            assert int((C.bits(t)[dead] != 0).sum()) == 0, tag
        # the locked rows did not move (their moments are zero unless given)
        if mkind == "zero":
            for a, b in zip(P, P0):
                assert torch.equal(C.bits(a)[locked], C.bits(b)[locked]), tag


def test_negative_zero_moment_makes_its_row_live():
    N = 130
    M = [torch.zeros(N, w, device=DEV) for w in C.WIDTHS]
    V = [torch.zeros(N, w, device=DEV) for w in C.WIDTHS]
    M[1][77, 5] = -0.0
    V[0][129, 2] = -0.0
    assert int(C.bits(M[1])[77, 5]) == -2 ** 31
    live = C.live_build(M, V, DEV)
    assert live.nonzero().flatten().tolist() == [77, 129]
    # and the step turns the stored -0.0 into +0.0, as the dense step does
    g = torch.Generator(device=DEV).manual_seed(3)
    P = [torch.randn(N, w, generator=g, device=DEV) for w in C.WIDTHS]
    G = [torch.zeros(N, w, device=DEV) for w in C.WIDTHS]
    rP, rM, rV, rG = ([t.clone() for t in ts] for ts in (P, M, V, G))
    C.reference_step(rP, rG, rM, rV, 0, torch.empty(0, dtype=torch.int64, device=DEV), step=1)
    stamp = torch.zeros(N, dtype=torch.int32, device=DEV)
    C.post_step(P, G, M, V, stamp, 1, live, 0, None, step=1)
    _assert_same("param", P, rP)
    _assert_same("exp_avg", M, rM)
    assert int(C.bits(M[1])[77, 5]) == 0


@pytest.mark.parametrize("N", [44, 4099])
def test_three_steps_touched_then_idle_and_never_touched(N):
    """A different touched set each step: rows = 0 mod 3, then rows = 1 mod 3, then the first row.  A
    row of the first set is touched, then idle with decaying moments; rows = 2 mod 3 are never
    touched and keep their bits and zero moments."""
    g = torch.Generator(device=DEV).manual_seed(N)
    none = torch.empty(0, dtype=torch.int64, device=DEV)
    P, M, V, _ = C.make_state(N, "zero", none, g, DEV)
    P0 = [t.clone() for t in P]
    rP, rM, rV = ([t.clone() for t in ts] for ts in (P, M, V))
    G = [torch.zeros(N, w, device=DEV) for w in C.WIDTHS]  # persistent: never re-zeroed by the test
    live = C.live_build(M, V, DEV)
    assert int(live.sum()) == 0
    stamp = torch.zeros(N, dtype=torch.int32, device=DEV)
    tail, anchors = 2, torch.tensor([3, 4, 3], device=DEV)
    sets = [torch.arange(0, N, 3, device=DEV), torch.arange(1, N, 3, device=DEV), torch.tensor([0], device=DEV)]
    for s, touched in enumerate(sets, start=1):
        vals = [torch.randn(touched.numel(), w, generator=g, device=DEV) for w in C.WIDTHS]
        rG = [torch.zeros(N, w, device=DEV) for w in C.WIDTHS]
        for gk, rk, v in zip(G, rG, vals):
            gk[touched] = v
            rk[touched] = v
        stamp[touched] = s
        C.reference_step(rP, rG, rM, rV, tail, anchors, step=s)
        C.post_step(P, G, M, V, stamp, s, live, tail, _lock_bytes(N, anchors), step=s)
        _assert_same((s, "param"), P, rP)
        _assert_same((s, "exp_avg"), M, rM)
        _assert_same((s, "exp_avg_sq"), V, rV)
        for t in G:
            assert int((C.bits(t) != 0).sum()) == 0, s
    never = torch.arange(2, N - tail, 3, device=DEV)
    assert int(live[never].sum()) == 0
    for a, b, m_ in zip(P, P0, M):
        assert torch.equal(C.bits(a)[never], C.bits(b)[never])
        assert int((C.bits(m_)[never] != 0).sum()) == 0
    idle = 6  # touched at step 1 only, unlocked: it kept moving at steps 2 and 3 on its decaying moments
    assert int(live[idle]) == 1 and not torch.equal(P[0][idle], P0[0][idle])


def test_mark_stamps_children_parents_and_skybox():
    """gsr_cut_mark_rows against the rows the blend's backward names: children, parents (-1 wraps to
    N - 1), the last S rows; nothing else."""
    import ctypes
    from diff_gaussian_rasterization import _lib
    N, R, S = 5000, 1200, 37
    g = torch.Generator(device=DEV).manual_seed(9)
    ri = torch.randperm(N - S, generator=g, device=DEV)[:R].int()
    pi = torch.randint(0, N - S, (R,), generator=g, device=DEV).int()
    pi[:5] = -1
    w = torch.rand(R, generator=g, device=DEV)
    for s_rows in (S, 0):
        stamp = torch.full((N,), 3, dtype=torch.int32, device=DEV)
        rc = _lib.load().gsr_cut_mark_rows(N, R, s_rows, ri.data_ptr(), pi.data_ptr(), w.data_ptr(), stamp.data_ptr(), 9,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, _lib.last_error()
        want = torch.full((N,), 3, dtype=torch.int32, device=DEV)
        want[ri.long()] = 9
        want[pi.long() % N] = 9
        want[N - s_rows:] = 9
        assert torch.equal(stamp, want)
        assert int(stamp[N - 1]) == 9  # a root's parent -1: the last row, skybox or not
