"""Inputs of the scaffold-selection and cloud-initialisation tests, shared by
tests/test_model_init_cpu.py (which asserts on the CPU that no selection case holds a row an fp32
evaluation could decide either way) and tests/test_gpu_model_init.py.  numpy only.

merge_cases(): Ps in {0, 1, 63, 64, 65, 255, 256, 257, 4099} x skybox counts {0, 1, Ps} where they
differ, rows spread over 0 .. 2.2 extents around a centre with fractional coordinates; plus

  none / all     nothing selected (every row inside 0.5 e) and everything selected (every row in the
                 ring), S = 0
  ties           centre (0, 0), so |x - cx| is exact: rows with m exactly 0.5 e and float32(1.5 e)
                 and one float32 on either side of each, in x and in y and with both signs; a NaN in
                 x, in y and in z (the z row once inside the ring, once outside: z is not read), an
                 Inf and a -Inf; the same rows once more below S.  The special rows sit across the
                 wave boundary at row 64.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
MERGE_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4099)
EXTENT = np.array([7.1, 5.0, 2.0], F32)  # 1.5 * float32(7.1) is not a float32: hi is rounded
CENTER = np.array([1.5, -2.25, 0.75], F32)


def _rows(rng, P, M=4):
    return [rng.normal(size=(P, 3)).astype(F32), rng.normal(size=(P, M, 3)).astype(F32),
            rng.normal(size=(P, 1)).astype(F32), rng.normal(size=(P, 3)).astype(F32),
            rng.normal(size=(P, 4)).astype(F32)]


def _case(name, seed, xyz, S, center=CENTER, extent=EXTENT, Pc=70, M=16):
    rng = np.random.default_rng(seed)
    sc = _rows(rng, xyz.shape[0])
    sc[0] = np.ascontiguousarray(xyz, F32)
    return dict(name=name, S=int(S), center=np.asarray(center, F32), extent=np.asarray(extent, F32), scaffold=sc,
                chunk=_rows(rng, Pc, M), M=M)


def _spread(rng, P, center=CENTER, extent=EXTENT, lo=0.0, hi=2.2):
    """Rows whose max(|dx|, |dy|) is uniform in [lo, hi] extents."""
    m = rng.uniform(lo, hi, P) * float(extent[0])
    other = rng.uniform(0, 1, P) * m
    sx, sy = rng.choice([-1.0, 1.0], P), rng.choice([-1.0, 1.0], P)
    in_x = rng.uniform(size=P) < 0.5
    dx = np.where(in_x, m, other) * sx
    dy = np.where(in_x, other, m) * sy
    return np.stack([center[0] + dx, center[1] + dy, rng.normal(size=P) * 3], 1).astype(F32)


def tie_rows(extent=EXTENT):
    """The special rows of the ties case around centre (0, 0, 0), and how many there are."""
    e0 = F32(extent[0])
    lo, hi = F32(F32(0.5) * e0), F32(F32(1.5) * e0)
    inf = F32(np.inf)
    edges = [lo, np.nextafter(lo, -inf), np.nextafter(lo, inf), hi, np.nextafter(hi, -inf), np.nextafter(hi, inf)]
    rows = []
    for v in edges:
        rows += [[v, 0.25, 1.0], [-v, -0.25, 1.0], [0.25, v, 1.0], [-0.25, -v, 1.0], [v, v, 1.0]]
    mid, out = F32(e0), F32(3.0) * e0
    rows += [[np.nan, mid, 0.0], [mid, np.nan, 0.0], [np.nan, np.nan, 0.0],
             [mid, 0.0, np.nan], [out, 0.0, np.nan], [0.0, 0.0, np.nan],      # z is not read
             [inf, 0.0, 0.0], [0.0, -inf, 0.0], [mid, mid, inf], [inf, np.nan, 0.0]]
    return np.array(rows, F32)


def merge_cases():
    cases = []
    for Ps in MERGE_SIZES:
        for S in sorted({0, 1, Ps}):
            if S > Ps:
                continue
            rng = np.random.default_rng(1000 + 7 * Ps + S)
            cases.append(_case(f"Ps{Ps}_S{S}", 2000 + 7 * Ps + S, _spread(rng, Ps), S,
                               Pc=(0 if Ps == 63 and S == 0 else 70), M=(4 if Ps == 65 else 16)))
    rng = np.random.default_rng(5)
    cases.append(_case("none_257", 6, _spread(rng, 257, hi=0.45), 0))
    cases.append(_case("all_257", 7, _spread(rng, 257, lo=0.55, hi=1.45), 0))
    cases.append(_case("none_no_chunk", 8, _spread(rng, 65, hi=0.45), 0, Pc=0))
    zero = np.zeros(3, F32)
    t = tie_rows()
    n = len(t)
    for S in (0, n + 40):
        # 40 ordinary rows, the special rows across the wave boundary at 64 (skybox rows when
        # S = n + 40), ordinary rows, then the special rows again past S
        xyz = np.concatenate([_spread(rng, 40, zero), t, _spread(rng, 150, zero), t, _spread(rng, 9, zero)])
        cases.append(_case(f"ties_S{S}", 9 + S, xyz, S, center=zero))
    return cases


INIT_N = (4, 5, 63, 64, 65, 257, 4099)
INIT_S = (0, 1, 64, 100)


def init_case(N, S, seed=None, zero_phi_row=False):
    """A cloud of N points whose centre lies within its radius of the origin (the bound on the
    skybox positions assumes it), colours in [0, 1], and S draw pairs with u_phi >= 2^-16."""
    rng = np.random.default_rng(100 * N + S if seed is None else seed)
    pts = (rng.normal(size=(N, 3)) * [6.0, 4.0, 1.5] + [0.7, -0.4, 0.2]).astype(F32)
    col = rng.uniform(0, 1, size=(N, 3)).astype(F32)
    u_theta = rng.uniform(0, 1, S).astype(F32)
    u_phi = np.maximum(rng.uniform(0, 1, S), 2.0 ** -16).astype(F32)
    u_theta[u_theta >= 1] = np.nextafter(F32(1), F32(0))
    u_phi[u_phi >= 1] = np.nextafter(F32(1), F32(0))
    if zero_phi_row and S:
        u_phi[S // 2] = 0.0
    return dict(points=pts, colors=col, u_theta=u_theta if S else None, u_phi=u_phi if S else None, N=N, S=S)
