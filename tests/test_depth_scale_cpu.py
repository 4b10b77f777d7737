"""CPU tests of the depth scale fit's restatement (tests/depth_scale_ref.py), its cases
(tests/depth_scale_cases.py) and the host side of gs_train/depth_scale.py: the restatement and the
line-by-line `literal` against the reference-generated tests/golden/depth_scale.npz, the distance between
the rule's s_mono and numpy's float32 pairwise mean (profiles/r24_depth_scale_margins.jsonl), the cases'
margins in exact arithmetic, the mutants the cases must notice
(profiles/r24_depth_scale_mutation_check.txt), and the exports and refusals without a GPU."""
from __future__ import annotations

import ctypes
import json
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import depth_scale_cases as C
import depth_scale_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "depth_scale.npz")
MARGINS = os.path.join(REPO, "profiles", "r24_depth_scale_margins.jsonl")
MUTATION = os.path.join(REPO, "profiles", "r24_depth_scale_mutation_check.txt")


def _fixture():
    g = np.load(GOLD)
    out = []
    for k in range(int(g["n"])):
        u16 = g[f"u16_{k}"] if int(g[f"has_map_{k}"]) else None
        args = (g[f"q_{k}"], g[f"t_{k}"], int(g[f"wh_{k}"][0]), int(g[f"wh_{k}"][1]), g[f"xy_{k}"], g[f"pid_{k}"],
                g["point_id"], g["point_xyz"], u16)
        out.append((k, args, g[f"ref_{k}"], bool(int(g[f"general_{k}"]))))
    return out


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def _sum_bound(n):
    """The relative error of an n-term fp64 sum of non-negative terms, any order, against the exact one."""
    return (n + 8) * 2.0 ** -52


def test_fixture_has_what_it_should():
    fx = _fixture()
    assert len(fx) >= 8
    refs = [ref for _, a, ref, _ in fx if a[8] is not None]
    assert any(np.isinf(r[0]) for r in refs) and sum(1 for r in refs if r[0] == 0 and r[1] == 0) >= 3
    assert sum(1 for r in refs if np.isfinite(r[0]) and r[0] > 0) >= 5
    assert any(a[8] is None for _, a, _, _ in fx) and sum(gen for *_, gen in fx) == 1


def test_literal_and_restatement_against_the_reference_fixture():
    """`literal` reproduces the reference's scale and offset exactly on every image whose transform is
    exact on any machine (rotations of entries 0, +-1, points on a 2^-8 grid): there no BLAS decides a
    bit.  The restatement has the same medians, exactly, and wherever its two mean absolute deviations
    equal `literal`'s (numpy sums pairwise, in float32 for s_mono) its scale and offset are the
    reference's to the last bit; elsewhere they lie within what the two sums' rounding explains.
    On the one image with a general rotation the reference went through a BLAS that fuses the transform's
    products (for more than a few rows, on the machine that made the fixture); the rule does not, so
    there the medians are held to the bound of that one rounding instead."""
    exact_and_fitted = 0
    rows = []
    for k, args, ref, general in _fixture():
        rule, lit = R.fit_image(*args), R.literal(*args)
        if args[8] is None:
            assert rule is None and lit is None
            continue
        if not general:
            assert _same([lit["scale"], lit["offset"]], ref), k
        assert rule["n_valid"] == lit["n_valid"], k
        n = max(rule["n_valid"], 1)
        if general:
            # |z_fused - z_rule| <= 3 ulps of the largest partial sum; |d inv| = |dz| / z^2; a median moves by at
            # most the largest change of an element, a mean absolute deviation by at most twice it
            q, t, _, _, _, pid, ids, xyz, _ = args
            Rm = R.qvec2rotmat(q)
            P = xyz  # every point of the table: a superset of the observed ones
            mag = np.abs(Rm[2, 0] * P[:, 0]) + np.abs(Rm[2, 1] * P[:, 1]) + np.abs(Rm[2, 2] * P[:, 2]) + abs(t[2])
            z = P @ Rm[2] + t[2]
            d = float(np.max(3 * 2.0 ** -53 * mag / z ** 2))
            assert abs(rule["t_colmap"] - lit["t_colmap"]) <= d, k
            assert abs(rule["s_colmap"] - lit["s_colmap"]) <= 2 * d + 2 * _sum_bound(n) * lit["s_colmap"], k
        else:
            assert rule["t_colmap"] == lit["t_colmap"], k
            assert abs(rule["s_colmap"] - lit["s_colmap"]) <= 2 * _sum_bound(n) * lit["s_colmap"], k
        assert rule["t_mono"] == lit["t_mono"], k
        # float32 pairwise summation of n terms and the division: (24 + ceil(log2 n)) float32 half-ulps ... the
        # bound of the issue, relative
        bound = (24 + math.ceil(math.log2(n))) * 2.0 ** -24
        rel = abs(rule["s_mono"] - lit["s_mono"]) / lit["s_mono"] if lit["s_mono"] else abs(rule["s_mono"])
        assert rel <= bound, (k, rel, bound)
        rows.append({"kind": "s_mono_rule_vs_numpy_f32", "image": k, "n": rule["n_valid"], "rel": rel, "bound": bound})
        if rule["s_mono"] == lit["s_mono"] and rule["s_colmap"] == lit["s_colmap"] and not general:
            assert _same([rule["scale"], rule["offset"]], ref), k
            exact_and_fitted += bool(rule["fitted"] and np.isfinite(ref[0]))
        elif not general and np.isfinite(ref[0]) and ref[0] != 0:
            e = rel + 2 * _sum_bound(n)
            assert abs(rule["scale"] - ref[0]) <= 2 * e * abs(ref[0]), k
            assert abs(rule["offset"] - ref[1]) <= 2 * e * (abs(rule["t_colmap"]) + abs(rule["t_mono"] * ref[0])), k
    assert exact_and_fitted >= 1  # a fitted image with finite outputs is among the exactly reproduced
    assert max(r["rel"] for r in rows) > 0  # and the deviation from numpy's float32 mean is there to be recorded
    os.makedirs(os.path.dirname(MARGINS), exist_ok=True)
    with open(MARGINS, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


def _exact_z(im, sc, missing):
    """Per masked observation the exact z (a Fraction; None for a non-finite point)."""
    Rm = R.qvec2rotmat(im["q"])
    assert set(np.abs(Rm[2]).tolist()) <= {0.0, 1.0}
    rows = {int(i): r for r, i in enumerate(sc["point_id"])}
    T = int(sc["point_id"].max()) + 1
    out = []
    for p in im["pid"].tolist():
        if not 0 <= p < T:
            continue
        if p in rows:
            X = sc["point_xyz"][rows[p]]
        elif missing == "origin":
            X = np.zeros(3)
        else:
            continue
        if not np.isfinite(X).all():
            out.append(None)
            continue
        out.append(sum((Fraction(float(Rm[2, j])) * Fraction(float(X[j])) for j in range(3)), Fraction(float(im["t"][2]))))
    return out


def test_cases_have_margins():
    """No case holds an observation or an image that fp64 could decide either way: in exact arithmetic
    every |z| >= 1e-6 and every |range - 1e-3| >= 1e-9.  (The validity comparisons are between fp32
    values the rule defines bit for bit: exact by construction.)"""
    closest = None
    for sc in C.scenes():
        for missing in C.MODES:
            for im in sc["images"]:
                zs = _exact_z(im, sc, missing)
                if not zs or any(z is None for z in zs):
                    continue
                assert all(abs(z) >= Fraction(1, 10 ** 6) for z in zs), (sc["name"], im["name"])
                inv = [1 / z for z in zs]
                gap = abs((max(inv) - min(inv)) - Fraction(1, 1000))
                assert gap >= Fraction(1, 10 ** 9), (sc["name"], im["name"], float(gap))
                closest = gap if closest is None else min(closest, gap)
    assert closest < Fraction(11, 10 ** 10)  # and the range cases do sit at 1e-6 relative from the threshold


def test_cases_cover_what_they_claim():
    Ccap = C.capacity()
    counts = {im["name"]: r for im, r in zip(C.by_name("counts")["images"], C.reference("counts"))}
    for n in (11, 12, 63, 64, 65, 255, 256, 257, Ccap - 1, Ccap, Ccap + 1, 3 * Ccap + 5):
        assert counts[f"n{n}"]["n_valid"] == n and counts[f"n{n}"]["fitted"]
    assert counts["n10"]["n_valid"] == 10 and not counts["n10"]["fitted"]
    assert counts["n0"]["n_valid"] == 0 and counts["all_minus_one"]["n_valid"] == 0
    assert counts[f"n{Ccap + 1}_of_{Ccap + 1 + (Ccap + 1) // 2 + 3}"]["n_valid"] == Ccap + 1
    d = {m: {im["name"]: r for im, r in zip(C.by_name("depths_ids_maps")["images"], C.reference("depths_ids_maps", m))}
         for m in C.MODES}
    o = d["origin"]
    assert not o["range_below_1e-3"]["fitted"] and o["range_below_1e-3"]["scale"] == 0
    assert o["range_above_1e-3"]["fitted"] and np.isnan(o["range_above_1e-3"]["scale"])  # 0 / 0
    assert o["range_from_valid_only_is_zero"]["s_colmap"] == 0 and o["range_from_valid_only_is_zero"]["fitted"]
    assert np.isinf(o["flat_map"]["scale"]) and np.isinf(o["flat_map"]["offset"]) and o["flat_map"]["offset"] < 0
    assert o["nan_point"]["nan_seen"] and not o["nan_point"]["fitted"]
    assert sum(r["nan_seen"] for r in o.values() if r) == 1  # seen by one image only
    assert o["absent_map"] is None and o["turned_round"]["n_valid"] == 0
    assert o["ids_in_gaps"]["n_valid"] == 16 and d["skip"]["ids_in_gaps"]["n_valid"] == 12
    assert o["only_gaps_and_ten"]["fitted"] and not d["skip"]["only_gaps_and_ten"]["fitted"]
    assert o["ids_at_and_above_T"]["n_valid"] == 12 and o["z_1e-6"]["fitted"] and o["behind_camera"]["n_valid"] == 13
    assert o["two_valued_tie_at_median"]["t_mono"] == float((np.float32(1000 / 65536) + np.float32(50000 / 65536)) / 2)
    assert {(sc["Hd"], sc["Wd"]) for sc in C.scenes()} >= {(6, 8), (48, 64)}
    assert {sc["Hd"] / sc["images"][0]["height"] for sc in C.scenes()} >= {1.0, 0.5, 2.0, 21 / 63}
    for name in ("positions_s1", "positions_s1_2", "positions_s2", "positions_s1_3"):
        p = {im["name"]: r for im, r in zip(C.by_name(name)["images"], C.reference(name))}
        assert p["zero_corner"]["n_valid"] == 18 and p["just_outside"]["n_valid"] == 14
        assert p["just_inside"]["n_valid"] == 17 and p["nan_and_inf"]["n_valid"] == 14
        assert p["ties_even_and_odd"]["n_valid"] == 18 and p["last_row_and_column"]["n_valid"] == 19
    sc = C.by_name("positions_s1_3")
    im = next(i for i in sc["images"] if i["name"] == "ties_even_and_odd")
    m = (im["xy"][-4:] * (sc["Hd"] / im["height"])).astype(np.float32) * np.float32(32)
    assert np.array_equal(m - np.floor(m), np.full((4, 2), 0.5, np.float32))  # exact ties, even and odd floors
    assert set((np.floor(m[:, 0]).astype(int) % 2).tolist()) == {0, 1}


def test_each_mutant_of_the_rule_changes_a_case():
    caught = {}
    for mutant in R.MUTANTS:
        for sc in C.scenes():
            for missing in C.MODES:
                for im, want in zip(sc["images"], C.reference(sc["name"], missing)):
                    got = R.fit_image(im["q"], im["t"], im["width"], im["height"], im["xy"], im["pid"], sc["point_id"],
                                      sc["point_xyz"], im["u16"], missing, mutant=mutant)
                    if want is not None and not all(_same(got[k], want[k]) for k in ("scale", "offset", "n_valid")):
                        caught.setdefault(mutant, []).append(f"{sc['name']}/{im['name']}[{missing}]")
    assert set(caught) == set(R.MUTANTS), set(R.MUTANTS) - set(caught)
    os.makedirs(os.path.dirname(MUTATION), exist_ok=True)
    with open(MUTATION, "w") as f:
        f.write("mutants of tests/depth_scale_ref.py fit_image and the cases whose scale, offset or n_valid they change\n")
        for mutant in R.MUTANTS:
            f.write(f"{mutant}: caught by {len(caught[mutant])}: {', '.join(caught[mutant][:6])}\n")


# ---- the C ABI and the wrapper without a GPU ----------------------------------------------------------

def test_lib_declares_and_exports_the_header_entry_points():
    from diff_gaussian_rasterization import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gsr_depth_scale.h")).read(), flags=re.S)
    decl = {m.group(1): len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
            for m in re.finditer(r"\b(gsr_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}
    assert set(decl) == {"gsr_depth_scale_lds_capacity", "gsr_depth_scale_scratch_bytes", "gsr_depth_scale_fit"}
    table = _lib.DEPTH_SCALE_SIGNATURES
    assert set(table) == set(decl)
    for name, n in decl.items():
        assert len(table[name][1]) == n, name
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in decl:
        assert hasattr(raw, name)
    assert _lib.load().gsr_abi_version() == _lib.ABI_VERSION == 7  # new entry points only
    from gs_train import depth_scale as D
    assert D.RECORD.itemsize == 56 and D.CAMERA_DOUBLES == 15


def test_calls_validate_without_gpu():
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    assert 256 <= L.gsr_depth_scale_lds_capacity() <= 160 * 1024 // 12
    assert L.gsr_depth_scale_scratch_bytes(0) == 0 and L.gsr_depth_scale_scratch_bytes(-3) == 0
    assert L.gsr_depth_scale_scratch_bytes(1000) >= 12 * 1000
    names = ("M", "cams", "off", "L", "index", "O", "xy", "pid", "N", "T", "table", "xyz", "K", "Hd", "Wd", "maps",
             "missing", "scratch", "records", "stream")
    dflt = dict(M=1, L=0, O=0, N=0, T=0, K=1, Hd=4, Wd=4, missing=0)
    args = lambda **kw: [kw.get(k, dflt.get(k)) for k in names]
    for kw in (dict(M=-1), dict(M=1 << 31), dict(L=-1), dict(N=1 << 31), dict(T=1 << 31), dict(K=-1), dict(missing=2),
               dict(Hd=0), dict(Wd=0), dict(L=5, O=3), dict()):  # the last: NULL pointers
        assert L.gsr_depth_scale_fit(*args(**kw)) == -1, kw  # GSR_ERR_INVALID_ARGUMENT
        assert b"gsr_depth_scale_fit" in L.gsr_last_error()
    assert L.gsr_depth_scale_fit(*args(M=0)) == 0  # nothing to do


def test_wrapper_refuses_bad_arguments_without_gpu():
    import torch
    from gs_train import depth_scale as D
    sc = C.by_name("depths_ids_maps")
    q, t, sizes, ptr, xy, pid, maps, index = C.arrays(sc)
    good = dict(qvecs=q, tvecs=t, sizes=sizes, obs_ptr=ptr, obs_xy=xy, obs_point_id=pid, point_id=sc["point_id"],
                point_xyz=sc["point_xyz"], maps=maps, map_index=index)

    def refused(match=None, **kw):
        a = dict(good)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            D.fit_depth_scales(**a)

    refused("obs_xy", obs_xy=xy.astype(np.float32))                      # wrong dtypes
    refused("obs_point_id", obs_point_id=pid.astype(np.int32))
    refused("point_id", point_id=sc["point_id"].astype(np.int32))
    refused("point_xyz", point_xyz=torch.from_numpy(sc["point_xyz"]).float())
    refused("qvecs", qvecs=q.astype(np.float32))
    refused("sizes", sizes=sizes.astype(np.float64))
    refused("maps", maps=maps.astype(np.float32))
    refused("obs_ptr", obs_ptr=ptr.astype(np.int32))
    bad = ptr.copy()
    bad[3], bad[4] = ptr[4], ptr[3]
    refused("obs_ptr", obs_ptr=bad)                                      # not ascending
    off = np.array([0, 5, 3, 8], np.int64)
    refused("obs_offsets", cameras=np.arange(3), map_index=index[:3], obs_index=np.arange(8), obs_offsets=off)
    refused("obs_offsets", cameras=np.arange(3), map_index=index[:3], obs_index=np.arange(8),
            obs_offsets=np.array([0, 3, 5, 9], np.int64))                # does not end at len(obs_index)
    refused("both or neither", obs_index=np.arange(8))
    refused("map_index", map_index=np.where(index == 2, len(maps), index))   # a map index out of range
    refused("map_index", map_index=np.where(index == 2, -2, index))
    refused("map_index", map_index=index[:-1])
    refused("maps", map_index=None)                                      # 15 maps for 16 cameras
    refused("Hd, Wd", maps=np.zeros((len(maps), 0, 8), np.uint16))       # Hd or Wd of 0
    refused("Hd, Wd", maps=np.zeros((len(maps), 6, 0), np.uint16))
    refused("cameras", cameras=np.array([0, len(q)]))
    refused("missing", missing="zero")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            D.fit_depth_scales(**good)
    # the camera table is R (row-major), t, width, height, map index
    tab = D.camera_table(q[:2], t[:2], sizes[:2], index[:2])
    assert tab.shape == (2, 15) and np.array_equal(tab[1, :9], R.qvec2rotmat(q[1]).reshape(9))
    assert np.array_equal(tab[:, 9:12], t[:2]) and np.array_equal(tab[:, 12:], np.c_[sizes[:2], index[:2]])
