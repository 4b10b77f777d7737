"""CPU tests of the coarse scaffold stage's front: the new C entry points are exported and typed
(ABI still 7), the wrappers validate before any GPU work, the scaffold files round-trip on the host,
tests/model_init_ref.py agrees with the reference's own create_from_pcd
(tests/golden/model_init.npz, made by tests/golden/make_model_init_golden.py), and no selection case
of tests/model_init_cases.py holds a row an fp32 evaluation could decide either way."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import model_init_cases as C
import model_init_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
HEADER = os.path.join(REPO, "include", "gsr_model_init.h")


# ---- the C boundary ----

def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(2): (m.group(1), m.group(3)) for m in
            re.finditer(r"\b(int|size_t)\s+(gsr_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_abi_version_stays_and_symbols_are_exported():
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    assert L.gsr_abi_version() == 7 == _lib.ABI_VERSION
    decl = _declared()
    table = _lib.MODEL_INIT_SIGNATURES
    assert set(decl) == set(table) == {"gsr_model_init_scratch_bytes", "gsr_model_init_cloud",
                                       "gsr_scaffold_merge_scratch_bytes", "gsr_scaffold_merge_count",
                                       "gsr_scaffold_merge_write"}
    raw = ctypes.CDLL(_lib.LIB_PATH)
    others = (set(_lib.SIGNATURES) | set(_lib.GT_SIGNATURES) | set(_lib.EVAL_SIGNATURES)
              | set(_lib.HIER_BUILD_SIGNATURES) | set(_lib.HIER_MERGE_SIGNATURES) | set(_lib.LPIPS_SIGNATURES))
    assert not set(table) & others
    for name, (res, args) in table.items():
        assert hasattr(raw, name), name
        ret, params = decl[name]
        params = [p.strip() for p in params.split(",")]
        assert len(params) == len(args), (name, len(params), len(args))
        assert res is (ctypes.c_size_t if ret == "size_t" else ctypes.c_int), name
        for p, a in zip(params, args):  # the documented signature, argument by argument
            if "*" in p:
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)), (name, p)
            elif p.startswith("int64_t"):
                assert a is ctypes.c_int64, (name, p)
            else:
                assert p.startswith("int ") and a is ctypes.c_int, (name, p)


def test_scratch_sizes_and_argument_checks_without_gpu():
    """Host arithmetic and the argument checks that come before any device work."""
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    ERR = -1  # GSR_ERR_INVALID_ARGUMENT
    assert L.gsr_model_init_scratch_bytes(0, 0) == 0 and L.gsr_model_init_scratch_bytes(5, -1) == 0
    assert L.gsr_model_init_scratch_bytes(1 << 31, 0) == 0
    prev = 0
    for n in (1, 4, 1000, 1 << 20):
        b = L.gsr_model_init_scratch_bytes(n, 100)
        assert b >= 4 * (n + 100) + L.gsr_knn_scratch_bytes(n + 100) and b >= prev
        prev = b
    assert L.gsr_scaffold_merge_scratch_bytes(-1) == 0
    assert L.gsr_scaffold_merge_scratch_bytes(0) > 0
    assert L.gsr_scaffold_merge_scratch_bytes(1 << 20) >= 4 * (1 << 20) + 16 * (1 << 14)
    one = ctypes.c_void_p(256)  # never dereferenced: the calls fail on their sizes / modes
    b4 = (ctypes.c_float * 4)()
    bad_init = [dict(N=0), dict(S=-1), dict(M=0), dict(M=17), dict(mode=1, S=0), dict(mode=0, S=3), dict(mode=2)]
    for kw in bad_init:
        a = dict(N=8, S=0, M=16, mode=0)
        a.update(kw)
        rc = L.gsr_model_init_cloud(a["N"], one, one, a["S"], one, one, a["M"], a["mode"], one, one, one, one, one, b4,
                                    one, None)
        assert rc == ERR and b"gsr_model_init_cloud" in L.gsr_last_error(), kw
    assert L.gsr_model_init_cloud(8, None, one, 0, None, None, 16, 0, one, one, one, one, one, b4, one, None) == ERR
    c3 = (ctypes.c_float * 3)(0, 0, 0)
    assert L.gsr_scaffold_merge_count(-1, 0, one, c3, c3, one, one, None) == ERR
    assert L.gsr_scaffold_merge_count(4, -1, one, c3, c3, one, one, None) == ERR
    assert L.gsr_scaffold_merge_count(4, 0, one, None, c3, one, one, None) == ERR
    assert b"gsr_scaffold_merge_count" in L.gsr_last_error()
    w = lambda Ps, K, Pc, M: L.gsr_scaffold_merge_write(Ps, K, one, one, one, one, one, Pc, M, one, one, one, one, one,
                                                        one, one, one, one, one, one, None)
    assert w(4, 5, 0, 16) == ERR and w(4, -1, 0, 16) == ERR and w(4, 1, -1, 16) == ERR
    assert w(4, 1, 1, 3) == ERR and w(4, 1, 1, 17) == ERR
    assert b"gsr_scaffold_merge_write" in L.gsr_last_error()


# ---- the Python wrappers ----

def _cloud(n=8):
    g = torch.Generator().manual_seed(0)
    return torch.randn(n, 3, generator=g), torch.rand(n, 3, generator=g)


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from gs_train import model_init as MI
    from gs_train.scaffold import Scaffold
    pts, col = _cloud()
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        MI.create_from_cloud(pts, col, 3, 1.0)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        MI.init_cloud(pts, col)
    with pytest.raises(ValueError, match="scaffold and bounds come together"):
        MI.create_from_cloud(pts, col, 3, 1.0, bounds=([0, 0, 0], [1, 1, 1]))
    sc = Scaffold(torch.zeros(2, 3), torch.zeros(2, 4, 3), torch.zeros(2, 1), torch.zeros(2, 3), torch.zeros(2, 4), 1)
    with pytest.raises(ValueError, match="scaffold and bounds come together"):
        MI.create_from_cloud(pts, col, 3, 1.0, scaffold=sc)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        MI.scaffold_merge(sc, [0, 0, 0], [1, 1, 1], (pts, torch.zeros(8, 16, 3), torch.zeros(8, 1), pts, torch.zeros(8, 4)))
    with pytest.raises(TypeError):
        MI.create_from_cloud(pts.numpy(), col, 3, 1.0)
    with pytest.raises(ValueError, match="skybox_points"):
        MI.create_from_cloud(pts, col, 3, 1.0, skybox_points=-1)


def test_rows_check_names_dtype_and_shape(monkeypatch):
    from gs_train import model_init as MI
    monkeypatch.setattr(MI, "require_gpu", lambda *t: None)  # reach the checks behind the device check
    with pytest.raises(ValueError, match="points: expected float32"):
        MI._rows("points", torch.zeros(8, 3, dtype=torch.float64), 3)
    with pytest.raises(ValueError, match=r"colors: expected shape \(N, 3\)"):
        MI._rows("colors", torch.zeros(8, 4), 3)
    with pytest.raises(ValueError, match="one row per point"):
        MI.init_cloud(torch.zeros(8, 3), torch.zeros(7, 3))
    with pytest.raises(ValueError, match="u_theta and u_phi come together"):
        MI.init_cloud(torch.zeros(8, 3), torch.zeros(8, 3), u_theta=torch.zeros(2))
    with pytest.raises(ValueError, match="the same length"):
        MI.init_cloud(torch.zeros(8, 3), torch.zeros(8, 3), u_theta=torch.zeros(2), u_phi=torch.zeros(3))
    with pytest.raises(ValueError, match="the cloud is empty"):
        MI.init_cloud(torch.zeros(0, 3), torch.zeros(0, 3))


def test_coarse_step_refuses_depth_and_scaffold():
    from gs_train.coarse import CoarseTrainStep
    with pytest.raises(ValueError, match="no depth supervision"):
        CoarseTrainStep(None, [], [], 8, 8, mono_invdepths=[None])
    with pytest.raises(ValueError, match="none of its own"):
        CoarseTrainStep(None, [], [], 8, 8, scaffold_points=3)


# ---- the scaffold files, on the host ----

def _host_model(P=37, M=4, seed=3):
    from gs_train.model_init import gaussians_from_raw
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return gaussians_from_raw(r(P, 3), r(P, M, 3), r(P, 1), r(P, 3), r(P, 4), n_images=2)


def _header_and_rows(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    return lines, data[end:]


def test_ply_layout_and_round_trip(tmp_path):
    from gs_train.scaffold import load_scaffold, ply_attributes, save_scaffold
    g = _host_model()
    save_scaffold(tmp_path / "sc", g, 5)
    lines, body = _header_and_rows(tmp_path / "sc" / "point_cloud.ply")
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 37"]
    want = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(9)]
            + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])
    assert ply_attributes(4) == want
    assert lines[3:-1] == [f"property float {n}" for n in want] and lines[-1] == "end_header"
    rows = np.frombuffer(body, "<f4").reshape(37, len(want))
    f = g._features.detach().numpy()
    np.testing.assert_array_equal(rows[:, 0:3], g._xyz.detach().numpy())
    assert not rows[:, 3:6].any()  # normals
    np.testing.assert_array_equal(rows[:, 6:9], f[:, 0])
    for c in range(3):  # f_rest is channel-major: f_rest_{3 c + k} = coefficient k + 1 of channel c
        for k in range(3):
            np.testing.assert_array_equal(rows[:, 9 + 3 * c + k], f[:, 1 + k, c])
    assert open(tmp_path / "sc" / "pc_info.txt").read() == "5"
    sc = load_scaffold(tmp_path / "sc", device="cpu")
    assert sc.skybox_points == 5 and sc.shs.shape == (37, 4, 3)
    for a, b in ((sc.xyz, g._xyz), (sc.shs, g._features), (sc.opacity_raw, g._opacity), (sc.log_scales, g._scaling),
                 (sc.rotations, g._rotation)):
        assert a.dtype == torch.float32 and torch.equal(a, b.detach())
    sky = sc.skybox_rows()
    assert [tuple(t.shape) for t in sky] == [(5, 3), (5, 3), (5, 4), (5, 1), (5, 4, 3)]
    assert torch.equal(sky[3], torch.sigmoid(g._opacity.detach()[:5]))  # activated, as create_from_hier takes them


def _rewrite(src, dst, order=None, type_name="float", ascii_=False):
    """The same vertex rows with the properties in another order / spelling / encoding."""
    lines, body = _header_and_rows(src / "point_cloud.ply")
    names = [ln.split()[2] for ln in lines if ln.startswith("property")]
    rows = np.frombuffer(body, "<f4").reshape(-1, len(names))
    order = list(range(len(names))) if order is None else order
    os.makedirs(dst, exist_ok=True)
    head = ["ply", "format ascii 1.0" if ascii_ else "format binary_little_endian 1.0", "comment rewritten",
            f"element vertex {rows.shape[0]}"] + [f"property {type_name} {names[i]}" for i in order] + ["end_header"]
    with open(dst / "point_cloud.ply", "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        if ascii_:
            for r in rows[:, order]:
                f.write((" ".join(repr(float(v)) for v in r) + "\n").encode())
        else:
            f.write(np.ascontiguousarray(rows[:, order]).tobytes())
    open(dst / "pc_info.txt", "w").write(open(src / "pc_info.txt").read() + "\n")


@pytest.mark.parametrize("variant", ["shuffled", "float32", "ascii"])
def test_ply_variants_load_the_same(tmp_path, variant):
    from gs_train.scaffold import load_scaffold
    save = tmp_path / "a"
    from gs_train.scaffold import save_scaffold
    save_scaffold(save, _host_model(), 2)
    ref = load_scaffold(save, device="cpu")
    n = 26
    order = list(np.random.default_rng(1).permutation(n)) if variant == "shuffled" else None
    _rewrite(save, tmp_path / "b", order=order, type_name="float32" if variant == "float32" else "float",
             ascii_=variant == "ascii")
    got = load_scaffold(tmp_path / "b", device="cpu")
    assert got.skybox_points == 2
    for f in ("xyz", "shs", "opacity_raw", "log_scales", "rotations"):
        assert torch.equal(getattr(got, f), getattr(ref, f)), f


def test_ply_errors_name_the_file(tmp_path):
    from gs_train.scaffold import load_scaffold, save_scaffold
    d = tmp_path / "a"
    save_scaffold(d, _host_model(), 2)
    path = d / "point_cloud.ply"
    whole = open(path, "rb").read()
    open(path, "wb").write(whole[:-5])
    with pytest.raises(ValueError, match=re.escape(f"{path}: truncated vertex data")):
        load_scaffold(d, device="cpu")
    for missing, what in (("opacity", "no property 'opacity'"), ("f_rest_4", "8 f_rest_"), ("rot_3", "4 rot_")):
        open(path, "wb").write(whole.replace(f"property float {missing}\n".encode(), b""))
        with pytest.raises(ValueError, match=re.escape(str(path)) + ".*" + re.escape(what)):
            load_scaffold(d, device="cpu")
    open(path, "wb").write(whole)
    open(d / "pc_info.txt", "w").write("many")
    with pytest.raises(ValueError, match="pc_info.txt"):
        load_scaffold(d, device="cpu")
    open(d / "pc_info.txt", "w").write("38")
    with pytest.raises(ValueError, match="outside the file's 37 rows"):
        load_scaffold(d, device="cpu")


def test_read_ply_xyz_reads_a_scaffold_file(tmp_path):
    """The shared header parser: the cloud reader takes the same file."""
    from gs_train.gtcloud import read_ply_xyz
    from gs_train.scaffold import save_scaffold
    g = _host_model()
    save_scaffold(tmp_path, g, 0)
    np.testing.assert_array_equal(read_ply_xyz(tmp_path / "point_cloud.ply"), g._xyz.detach().numpy())


# ---- the restatement against the reference's own run ----

def _ulps(a, b):
    a = np.asarray(a, np.float32)
    return np.abs(a.astype(np.float64) - np.asarray(b, np.float64)) / np.spacing(np.abs(a)).astype(np.float64)


def test_ref_matches_reference_create_from_pcd_skybox_mode():
    """model_init_ref.init_cloud against create_from_pcd(skybox_points=16, scaffold_file=""): exact
    where the reference is float32 arithmetic, within float32 rounding of the float64 formulas
    elsewhere (torch's float32 cos / sin / arccos / log chain: a few ulps of the result's scale)."""
    d = np.load(os.path.join(GOLD, "model_init.npz"))
    S = int(d["skybox_points"])
    assert S == 16 and d["u_theta"].shape == (S,) and d["u_phi"].shape == (S,)
    np.testing.assert_array_equal(R.knn_mean_dist2(d["skybox_xyz"]), d["skybox_dist2"])
    r = R.init_cloud(d["points"], d["colors"], d["u_theta"], d["u_phi"], M=4, dist2=d["skybox_dist2"])
    np.testing.assert_array_equal(d["skybox_xyz"][S:], d["points"])
    r10 = 10 * r["radius64"]
    assert np.abs(d["skybox_xyz"][:S] - r["xyz64"][:S]).max() <= r10 * 2.0 ** -20
    feat = np.concatenate([d["skybox_f_dc"], d["skybox_f_rest"]], 1)
    np.testing.assert_array_equal(feat, r["features"])
    np.testing.assert_array_equal(d["skybox_rotation"], r["rotation"])
    np.testing.assert_array_equal(d["skybox_opacity"][:S], np.float32(0.7))
    assert _ulps(d["skybox_opacity"][S:], r["opacity64"][S:]).max() <= 2
    assert np.abs(d["skybox_scaling"] - r["scaling64"]).max() <= 2.0 ** -22 * max(1, np.abs(r["scaling64"]).max())


def test_ref_matches_reference_create_from_pcd_scaffold_mode():
    d = np.load(os.path.join(GOLD, "model_init.npz"))
    assert int(d["scaffold_skybox_points"]) == 3
    chunk = R.init_cloud(d["points"], d["colors"], M=16, dist2=d["scaffold_dist2"])
    np.testing.assert_array_equal(R.knn_mean_dist2(d["points"]), d["scaffold_dist2"])
    K = int(d["scaffold_points"])
    sc = [d["scaffold_in_" + k] for k in ("xyz", "shs", "opacity", "scaling", "rotation")]
    # the chunk rows as the reference left them (its float32 log chain), so the merge is compared to the bit
    feat = np.concatenate([d["scaffold_f_dc"], d["scaffold_f_rest"]], 1)
    got = [d["scaffold_xyz"], feat, d["scaffold_opacity"], d["scaffold_scaling"], d["scaffold_rotation"]]
    ch = [g[K:] for g in got]
    out, K_ref, idx = R.scaffold_merge(sc, 3, d["center"], d["extent"], ch, M=16)
    assert K_ref == K and 3 < K < 40 and list(idx[:3]) == [0, 1, 2]
    assert not R.undecided(sc[0], 3, d["center"], d["extent"]).any()
    for a, b in zip(out, got):
        np.testing.assert_array_equal(a, b)
    assert not feat[:K, 4:].any()
    # and the chunk rows themselves: plain mode
    np.testing.assert_array_equal(ch[0], d["points"])
    np.testing.assert_array_equal(ch[1], chunk["features"])
    np.testing.assert_array_equal(ch[4], chunk["rotation"])
    assert _ulps(ch[2], chunk["opacity64"]).max() <= 2
    assert np.abs(ch[3] - chunk["scaling64"]).max() <= 2.0 ** -22 * max(1, np.abs(chunk["scaling64"]).max())


# ---- the selection cases ----

def test_merge_cases_cover_the_sizes_and_hold_no_undecided_row():
    cases = C.merge_cases()
    assert {c["scaffold"][0].shape[0] for c in cases} >= set(C.MERGE_SIZES)
    seen = set()
    undecided = total = 0
    for c in cases:
        xyz, S = c["scaffold"][0], c["S"]
        u = R.undecided(xyz, S, c["center"], c["extent"])
        undecided += int(u.sum())
        total += len(u)
        sel = R.scaffold_select(xyz, S, c["center"], c["extent"])
        Ps = len(sel)
        if Ps:
            seen.add("none" if not sel.any() else "all" if sel.all() else "some")
        assert sel[:S].all()
    assert undecided == 0, (undecided, total)  # the share of rows left out as undecided is 0
    assert seen == {"none", "all", "some"}


def test_tie_rows_decide_as_the_rule_says():
    t = C.tie_rows()
    sel = R.scaffold_select(t, 0, np.zeros(3, np.float32), C.EXTENT)
    # per edge value five rows; edges: lo, lo-, lo+, hi, hi-, hi+  -> only lo+ and hi- are inside
    assert sel[:30].reshape(6, 5).all(1).tolist() == [False, False, True, False, True, False]
    assert not sel[:30].reshape(6, 5)[[0, 1, 3, 5]].any()
    # NaN x, NaN y, both; NaN z inside, NaN z outside, NaN z at the centre; Inf, -Inf, Inf z inside, Inf + NaN
    assert sel[30:].tolist() == [False, False, False, True, False, False, False, False, True, False]
    assert float(np.float32(1.5) * C.EXTENT[0]) != 1.5 * float(C.EXTENT[0])  # hi is a rounded product
    assert R.scaffold_select(t, len(t), np.zeros(3, np.float32), C.EXTENT).all()
