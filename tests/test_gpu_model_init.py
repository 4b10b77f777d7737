"""GPU tests of csrc/model_init.hip (include/gsr_model_init.h) through gs_train.model_init, against
tests/model_init_ref.py: the scaffold selection and merge to the bit at the compaction's edge sizes
and at the predicate's ties, and the model from a cloud -- exact where the reference is float32
arithmetic, within bounds derived from the operations elsewhere (each test's docstring)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import gs_oracle as O
import model_init_cases as C
import model_init_ref as R
from helpers import record_margins

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same_bits(a, b, what):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    assert a.shape == b.shape, (what, a.shape, b.shape)
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


# ---- scaffold selection and merge ----

MERGE = {c["name"]: c for c in C.merge_cases()}


@pytest.mark.parametrize("name", sorted(MERGE))
def test_scaffold_merge_is_bit_exact(name):
    """K, the selected rows in their order, every copied value (NaN and Inf payloads included), the
    zero padding of coefficients 4.., and the chunk rows behind them: to the bit.  The cases hold no
    row an fp32 evaluation could decide either way (asserted on the CPU,
    test_merge_cases_cover_the_sizes_and_hold_no_undecided_row)."""
    from gs_train.model_init import scaffold_merge
    from gs_train.scaffold import Scaffold
    c = MERGE[name]
    want, K, idx = R.scaffold_merge(c["scaffold"], c["S"], c["center"], c["extent"], c["chunk"], M=c["M"])
    s = c["scaffold"]
    sc = Scaffold(_t(s[0]), _t(s[1]), _t(s[2]), _t(s[3]), _t(s[4]), c["S"])
    got, K_gpu = scaffold_merge(sc, c["center"], c["extent"], tuple(_t(a) for a in c["chunk"]))
    assert K_gpu == K
    Pc = c["chunk"][0].shape[0]
    for g, w, what in zip(got, want, ("xyz", "features", "opacity", "scaling", "rotation")):
        assert g.shape[0] == K + Pc
        _same_bits(g, w, f"{name} {what}")
    assert not got[1][:K, 4:].any()
    # the order: the scaffold's xyz rows are distinct, so the copied rows name their sources
    _same_bits(got[0][:K], s[0][idx], "selected rows in order")


def test_scaffold_merge_count_matches_a_4099_row_wave_pattern():
    """Selected rows only at the wave edges (lanes 0 and 63 of every wave) of 4099 rows: the ballot's
    lane arithmetic and the scan over 65 waves."""
    from gs_train.model_init import scaffold_merge
    from gs_train.scaffold import Scaffold
    Ps = 4099
    rng = np.random.default_rng(3)
    s = C._rows(rng, Ps)
    lane = np.arange(Ps) % 64
    s[0][:, :2] = 0.0
    s[0][(lane == 0) | (lane == 63), 0] = C.EXTENT[0]  # m = e: inside the ring
    ch = C._rows(rng, 3, 16)
    want, K, idx = R.scaffold_merge(s, 0, np.zeros(3, F32), C.EXTENT, ch)
    assert K == 65 + 64  # lane 0 of 65 waves (the last holds 3 rows), lane 63 of 64
    got, K_gpu = scaffold_merge(Scaffold(*[_t(a) for a in s], 0), np.zeros(3), C.EXTENT, tuple(_t(a) for a in ch))
    assert K_gpu == K
    for g, w in zip(got, want):
        _same_bits(g, w, "wave pattern")


# ---- the model from a cloud ----

def _run_init(case, M):
    from gs_train.model_init import init_cloud
    u = (None, None) if not case["S"] else (_t(case["u_theta"]), _t(case["u_phi"]))
    arrays, (mean, radius) = init_cloud(_t(case["points"]), _t(case["colors"]), u[0], u[1], M)
    return [a.cpu().numpy() for a in arrays], mean, radius


def _check_init(case, M, tag):
    """Exact and bounded checks of one gsr_model_init_cloud call; returns the margins (measured
    error over its bound, <= 1)."""
    (xyz, feat, op, sc, rot), mean, radius = _run_init(case, M)
    S, N = case["S"], case["N"]
    dist2 = O.knn_mean_dist2(xyz)  # the C oracle's, bit-exact with gsr_knn_mean_dist2 (test_gpu_knn.py)
    r = R.init_cloud(case["points"], case["colors"], case["u_theta"], case["u_phi"], M=M, dist2=dist2, radius=radius)
    # to the bit, against float32 numpy
    _same_bits(xyz[S:], case["points"], "cloud xyz")
    _same_bits(rot, r["rotation"], "rotation")
    _same_bits(feat, r["features"], "SH DC (a division) and the zero coefficients")
    _same_bits(mean, r["mean"], "mean")
    if S:
        _same_bits(op[:S], np.full((S, 1), 0.7, F32), "the raw 0.7")
    m = {}
    # radius: 3 ulp of the float64 norm
    m["radius_ulp3"] = abs(float(radius) - r["radius64"]) / (3 * float(np.spacing(F32(radius))))
    # logit constants: 2 ulp
    lg = op[S:].astype(np.float64)
    m["logit_ulp2"] = float((np.abs(lg - r["opacity64"][S:]) / (2 * np.spacing(np.abs(op[S:])).astype(np.float64))).max())
    # scaling: 2^-22 max(1, |ref|) absolute
    ref = r["scaling64"]
    fin = np.isfinite(ref)
    assert fin.all() or not S  # only a cloud of N < 4 has infinite distances, and it has no skybox here
    m["scaling"] = float((np.abs(sc.astype(np.float64) - ref)[fin] / (2.0 ** -22 * np.maximum(1, np.abs(ref[fin])))).max())
    assert np.array_equal(sc[:, 0], sc[:, 1]) and np.array_equal(sc[:, 0], sc[:, 2])
    if S:
        r10 = r["r10"]
        bound = r10 * (2.0 ** -22 + 2.0 ** -23 / np.maximum(r["sin_phi"], 1e-300))
        err = np.abs(xyz[:S].astype(np.float64) - r["xyz64"][:S])
        ok = r["sin_phi"] > 0
        m["skybox_xyz"] = float((err[ok] / bound[ok, None]).max()) if ok.any() else 0.0
        d = xyz[:S].astype(np.float64) - mean.astype(np.float64)
        m["skybox_dist"] = float((np.abs(np.sqrt((d * d).sum(1)) - r10)[ok] / bound[ok]).max()) if ok.any() else 0.0
        assert (d[:, 2] / r10 >= -0.4 - bound / r10).all()
        for k in np.nonzero(~ok)[0]:  # u_phi = 0: cos(phi) = 1 exactly
            want = np.array([mean[0], mean[1], F32(mean[2] + F32(F32(10.0) * F32(radius)))], F32)
            _same_bits(xyz[k], want, "u_phi = 0 row")
    record_margins(f"model_init_{tag}", **m)
    for k, v in m.items():
        assert v <= 1.0, (tag, k, v)
    return m


@pytest.mark.parametrize("S", C.INIT_S)
@pytest.mark.parametrize("N", C.INIT_N)
def test_init_cloud_sizes(N, S):
    """gsr_model_init_cloud at N x S, M = 16 (M = 4 where N is odd), bounds against float64:

    radius   3 ulp: three squares and two adds (each half an ulp of a sum of positives) and sqrt.
    logit    2 ulp: the constant is evaluated in float64 and rounded once (half an ulp).
    scaling  2^-22 max(1, |ref|) absolute: sqrt's one rounding (2^-24 relative) passes through the
             log as 2^-24 absolute; logf taken as 2 ulp (no accuracy table of the device library
             is at hand, so the figure is not replaced), at most 2^-23 |ref| for the typical ulp of
             2^-23.5 |ref|; the float32 store is inside logf's ulp.  The bound is not widened for a
             value just above a power of two, where 2 ulp alone would reach it: a miss there means
             logf is worse than 1.5 ulp on that input and is worth knowing.
    skybox position, per coordinate: 10 radius (2^-22 + 2^-23 / sin(phi)).  cos(phi) carries at most
             2^-23 and d sin / d cos = -cos / sin; the remaining 2^-22 covers the direction's
             rounding (2^-25), 10 * radius (2^-24), the product (2^-24) and the sum with the mean
             (2^-24 (|mean| + 10 radius)), given a cloud whose centre lies within its radius of the
             origin, as model_init_cases.init_case makes them.  The reference value is
             mean + 10 radius dir in float64 on the kernel's own float32 mean and radius (checked
             above on their own), with u_phi >= 2^-16.
    distance from the mean: the same bound; cos(phi) >= -0.4."""
    _check_init(C.init_case(N, S), 4 if N % 2 else 16, f"N{N}_S{S}")


def test_init_cloud_zero_phi_row_is_exact():
    """u_phi = 0: cos(phi) = 1 and sin(phi) = 0 exactly, so the row is mean + (0, 0, 10 radius)
    evaluated in float32, to the bit (checked inside _check_init for rows with sin(phi) = 0)."""
    case = C.init_case(257, 64, zero_phi_row=True)
    assert (case["u_phi"] == 0).sum() == 1
    _check_init(case, 16, "zero_phi")


def test_init_cloud_three_points_follow_the_knn_contract():
    """N = 3, plain mode: gsr_knn.h documents FLT_MAX for the missing third neighbour, so
    dist2 = (d0 + d1 + FLT_MAX) / 3 rounds to FLT_MAX / 3 and the scale is log(sqrt(that)), finite."""
    case = C.init_case(3, 0)
    (xyz, feat, op, sc, rot), mean, radius = _run_init(case, 16)
    d = O.knn_mean_dist2(xyz)
    assert (d == F32(np.finfo(F32).max) / F32(3)).all()
    want = np.log(np.sqrt(d.astype(np.float64)))
    assert np.abs(sc[:, 0] - want).max() <= 2.0 ** -22 * np.abs(want).max()
    assert np.isfinite(sc).all()
    _check_init(case, 16, "N3")


def test_create_from_cloud_draws_as_the_reference_does():
    """The public call: two torch.rand(S) draws from the device generator, theta first; the set is in
    the joined layout with the raw arrays as the kernel wrote them (no log / logit round trip)."""
    from gs_train.model_init import create_from_cloud, init_cloud
    case = C.init_case(257, 64)
    pts, col = _t(case["points"]), _t(case["colors"])
    torch.manual_seed(5)
    g, S, K = create_from_cloud(pts, col, n_images=3, spatial_lr_scale=2.5, skybox_points=64, sh_degree=1)
    torch.manual_seed(5)
    u_theta, u_phi = torch.rand(64, device=DEV), torch.rand(64, device=DEV)
    arrays, _ = init_cloud(pts, col, u_theta, u_phi, M=4)
    assert (S, K) == (64, None) and g.joined and g.P == 257 + 64 and g.active_sh_degree == 0
    assert g.spatial_lr_scale == 2.5 and g._exposure.shape == (3, 3, 4)
    for a, b in zip((g._xyz, g._features, g._opacity, g._scaling, g._rotation), arrays):
        assert torch.equal(a.detach(), b)
    assert g._features.shape == (321, 4, 3) and g.get_features is g._features
    assert float(g._opacity.detach()[0]) == float(F32(0.7))
    for t in (g.max_radii2D, g.xyz_gradient_accum, g.denom):
        assert t.shape[0] == 321 and not t.any()


def test_non_finite_cloud_is_refused_before_anything_is_written():
    """A NaN at point 7 and an Inf at point 3: GSR_ERR_INVALID_ARGUMENT naming point 3, and no
    output array touched."""
    from diff_gaussian_rasterization import _lib
    from gs_train._native import ptr, stream
    case = C.init_case(4099, 64)
    pts = case["points"].copy()
    pts[7, 1] = np.nan
    pts[3, 2] = np.inf
    pts[4000, 0] = -np.inf
    L = _lib.load()
    P = 4099 + 64
    outs = [torch.full((P, w), -7.5, device=DEV) for w in (3, 48, 1, 3, 4)]
    scratch = torch.empty(L.gsr_model_init_scratch_bytes(4099, 64), dtype=torch.uint8, device=DEV)
    b = (ctypes.c_float * 4)(1, 2, 3, 4)
    tp, tc, tu, tv = _t(pts), _t(case["colors"]), _t(case["u_theta"]), _t(case["u_phi"])
    rc = L.gsr_model_init_cloud(4099, ptr(tp), ptr(tc), 64, ptr(tu), ptr(tv), 16, 1, *[ptr(o) for o in outs], b,
                                ptr(scratch), stream(torch.device(DEV, 0)))
    torch.cuda.synchronize()
    assert rc == -1
    msg = _lib.last_error()
    assert "gsr_model_init_cloud" in msg and "cloud point 3 " in msg, msg
    assert all(bool((o == -7.5).all()) for o in outs) and list(b) == [1, 2, 3, 4]
    from gs_train.model_init import init_cloud
    with pytest.raises(RuntimeError, match="cloud point 3 has a NaN or Inf coordinate"):
        init_cloud(tp, tc, tu, tv)
