"""CPU tests of the LiDAR preparation (gs_train.lidar, include/gsr_lidar.h): tests/lidar_ref.py against
independent checks, the condition every case of tests/lidar_cases.py must meet (no point an fp32
evaluation could decide either way; the measured margins go to profiles/r17_lidar_margins.jsonl), the
ctypes table against the header, the argument checks and the PLY mesh reader."""
from __future__ import annotations

import ctypes
import json
import os
import re
import struct

import numpy as np
import pytest

import lidar_cases as C
import lidar_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "gsr_lidar.h")
MARGINS = os.path.join(REPO, "profiles", "r17_lidar_margins.jsonl")


# ---- the reference against independent checks ----------------------------------------------------

def _sampled_distance(p, tri, n=400):
    """The distance from p to the closest of (n + 1)(n + 2) / 2 barycentric samples of tri: an upper
    bound of the true distance, above it by less than the sample pitch."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = i + j <= n
    u, v = i[keep] / n, j[keep] / n
    q = tri[0] + u[:, None] * (tri[1] - tri[0]) + v[:, None] * (tri[2] - tri[0])
    return np.sqrt(((q - p) ** 2).sum(1).min())


@pytest.mark.parametrize("name", ["features", "degenerate", "needles"])
def test_distance_reference_against_dense_sampling(name):
    c = C.mesh_case(name)
    v, f = c["vertices"].astype(np.float64), c["faces"]
    rng = np.random.default_rng(0)
    rows = rng.choice(len(c["points"]), size=min(40, len(c["points"])), replace=False)
    for r in rows:
        p = c["points"][r].astype(np.float64)
        d = np.sqrt(R.min_d2(c["points"][r:r + 1], c["vertices"], c["faces"])[0])
        s = min(_sampled_distance(p, v[t]) for t in f)
        pitch = max(np.abs(v[t] - v[t][0]).max() for t in f) / 400 * 2
        assert d <= s + 1e-12, (name, r, d, s)  # the samples lie on the triangles
        assert s - d <= pitch, (name, r, d, s)   # and one of them within a pitch of the closest point


def test_distance_reference_on_placed_points():
    """feature_points places each point at a known distance from its triangle."""
    tri = C.TRI.astype(np.float32).astype(np.float64)
    pts = C.feature_points(tri)  # float64, not yet cast
    v, f = tri.astype(np.float32), np.array([[0, 1, 2]])
    d2, _, _ = R.pair_d2(pts[:, None, :].astype(np.float32), v[None, 0], v[None, 1], v[None, 2], np.float64)
    d = np.sqrt(d2[:, 0])
    n = (len(pts) - 2) // 2
    assert np.allclose(d[:n], C.MAX_DISTANCE * (1 - C.DELTA), rtol=0, atol=2e-7)
    assert np.allclose(d[n:2 * n], C.MAX_DISTANCE * (1 + C.DELTA), rtol=0, atol=2e-7)
    assert np.all(d[2 * n:] <= 2e-7)


def _dict_voxel_mean(points, colors, s):
    p = points.astype(np.float64)
    o = p.min(0) - s / 2
    cells = {}
    for r, q in enumerate(p):
        cells.setdefault(tuple(int(np.floor((q[k] - o[k]) / s)) for k in range(3)), []).append(r)
    keys = sorted(cells, key=lambda k: (k[2], k[1], k[0]))
    means = np.array([p[cells[k]].mean(0) for k in keys])
    cm = None if colors is None else np.array([colors[cells[k]].astype(np.float64).mean(0) for k in keys])
    return np.array(keys), means, cm, np.array([len(cells[k]) for k in keys])


@pytest.mark.parametrize("name", C.VOXEL_CASES)
def test_voxel_reference_against_a_dictionary(name):
    pts, col, s = C.voxel_case(name)
    means, cmeans, counts, ijk = R.voxel_mean(pts, col, s)
    keys, dmeans, dcm, dcounts = _dict_voxel_mean(pts, col, s)
    assert np.array_equal(ijk, keys) and np.array_equal(counts, dcounts)
    assert counts.sum() == len(pts)
    assert R.ulp_diff(means, dmeans.astype(np.float32)).max() <= 1
    if col is not None:
        assert R.ulp_diff(cmeans, dcm.astype(np.float32)).max() <= 1
    if name == "one_point":
        assert np.array_equal(means, pts) and counts.tolist() == [1]
    if name == "one_voxel":
        assert len(counts) == 1
    if name == "run_lengths":
        assert sorted(counts.tolist()) == [1, 64, 65, 3000]
    if name == "on_faces":  # a point on a face is the upper voxel's; the one 2^-20 below it the lower one's
        on = np.isin(pts[:, 1], (0.125 + 0.25 * np.arange(9)).astype(np.float32))
        j = np.floor((pts[:, 1].astype(np.float64) + 0.125) / 0.25)
        assert np.array_equal(j[on], np.round((pts[on, 1] + 0.125) / 0.25)) and on.sum() > 200


def test_voxel_reference_rejects_a_voxel_size_too_small():
    pts, s = C.REJECTED_VOXEL
    with pytest.raises(ValueError):
        R.voxel_mean(pts, None, s)


# ---- the condition on the cases ------------------------------------------------------------------

def test_no_case_holds_a_point_fp32_could_decide_either_way():
    """The largest gap between the fp32 restatement of the kernel's arithmetic and float64, over every
    point of every case (as a distance), is measured here and written to
    profiles/r17_lidar_margins.jsonl.  The band is 4x that gap (the margin of
    profiles/r12_shape_margins.jsonl), or the rounding bound 12 * 2^-24 * L if that is larger.  L bounds
    the differences v - p the evaluation of a pair forms when the pair is anywhere near a threshold:
    the largest queried distance plus the largest triangle's diameter.  About a dozen roundings reach
    the distance (the differences, two per dot product, the division, the normal's compensated
    products), each relative to a length no larger than L; a pair farther than that is far from every
    threshold by more than any such error.  No point may have a float64 distance within the band of
    any queried max_distance.  A condition on the inputs, not a tolerance: the GPU test then asks for
    the float64 mask exactly."""
    rows, worst_gap, worst_L = [], 0.0, 0.0
    dist = {}
    for name in C.MESH_CASES:
        c = C.mesh_case(name)
        d64 = np.sqrt(C.mesh_case_d2(name))
        d32 = np.sqrt(R.min_d2(c["points"], c["vertices"], c["faces"], np.float32).astype(np.float64))
        ok = np.isfinite(c["points"]).all(1)
        gap = float(np.abs(d32[ok] - d64[ok]).max()) if ok.any() else 0.0
        t = c["vertices"].astype(np.float64)[c["faces"]]
        L = max(C.QUERY_DISTANCES) + float(np.sqrt(((t - t[:, [1, 2, 0]]) ** 2).sum(-1)).max())
        dist[name] = d64[ok]
        rows.append({"case": name, "points": int(len(c["points"])), "triangles": int(len(c["faces"])),
                     "gap_m": gap, "reach_plus_diameter_m": L})
        worst_gap, worst_L = max(worst_gap, gap), max(worst_L, L)
    band = max(4 * worst_gap, 12 * R.F32_EPS * worst_L)
    inside = 0
    for row in rows:
        d = dist[row["case"]]
        row["band_m"] = band
        for q in C.QUERY_DISTANCES:
            k = int((np.abs(d - q) <= band).sum()) if len(d) else 0
            row[f"inside_{q}"] = k
            row[f"closest_{q}_m"] = float(np.abs(d - q).min()) if len(d) else None
            inside += k
    os.makedirs(os.path.dirname(MARGINS), exist_ok=True)
    with open(MARGINS, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    assert band < C.GUARD and band < C.MAX_DISTANCE * C.DELTA, band  # what the placement keeps clear
    assert inside == 0, [r for r in rows if any(r[f"inside_{q}"] for q in C.QUERY_DISTANCES)]


@pytest.mark.parametrize("name", C.MESH_CASES)
def test_fp32_restatement_decides_as_float64(name):
    """What the condition buys: the kernel's rule, restated in fp32 with its sep test, gives the
    float64 mask on every case and queried distance."""
    c = C.mesh_case(name)
    bounds = R.crop_bounds(*c["box"]) if c["box"] else None
    for q in C.QUERY_DISTANCES:
        want = R.near_mask(c["points"], C.mesh_case_d2(name), q, bounds)
        assert np.array_equal(R.near_mask_f32(c["points"], c["vertices"], c["faces"], q, bounds), want), (name, q)


def test_cases_cover_what_they_claim():
    names = set(C.MESH_CASES)
    assert {int(re.search(r"_P(\d+)_", n).group(1)) for n in names if n.startswith("sizes")} == set(C.POINT_COUNTS)
    assert {int(re.search(r"_F(\d+)", n).group(1)) for n in names if n.startswith("sizes")} == set(C.TRIANGLE_COUNTS)
    for n in names:
        c = C.mesh_case(n)
        assert len(c["points"]) <= 4099 and len(c["faces"]) <= 5000
    assert len(C.mesh_case("fan")["faces"]) == 5000
    p = C.mesh_case("placement")
    b = R.crop_bounds(*p["box"])
    on = np.isin(p["points"][:, 0], b[:2]) | np.isin(p["points"][:, 1], b[2:])
    assert on.sum() >= 80 and not R.crop_mask(p["points"], b)[on].any()
    assert (~np.isfinite(p["points"]).all(1)).sum() >= 10
    # on both sides of the threshold, and kept and dropped points in every larger case
    for n in ("features", "neighbour_cells", "oversize", "degenerate", "needles", "shifted", "placement", "fan"):
        m = R.near_mask(C.mesh_case(n)["points"], C.mesh_case_d2(n), C.MAX_DISTANCE)
        assert m.any() and (~m).any(), n
    assert np.array_equal(R.near_mask(C.TIE_CASE["points"],
                                      R.min_d2(C.TIE_CASE["points"], C.TIE_CASE["vertices"], C.TIE_CASE["faces"]),
                                      C.TIE_DISTANCE), C.TIE_EXPECTED)
    assert np.array_equal(R.near_mask_f32(C.TIE_CASE["points"], C.TIE_CASE["vertices"], C.TIE_CASE["faces"],
                                          C.TIE_DISTANCE), C.TIE_EXPECTED)


@pytest.mark.parametrize("F", C.ONE_CELL_COUNTS)
def test_one_cell_cases_are_what_they_claim(F):
    """The mesh fits under the cell edge of an index built for MAX_DISTANCE; in every point set and at
    every queried distance the reference makes both decisions, the last triangle alone is in reach of
    the near points, no distance is within GUARD of a threshold and the fp32 restatement agrees."""
    c = C.one_cell_case(F)
    v, f = c["vertices"], c["faces"]
    assert len(f) == F and (v.max(0) - v.min(0)).max() < 2 * C.MAX_DISTANCE
    assert c["points"].shape == (3, 65, 3)
    for k, pts in enumerate(c["points"]):
        d2 = R.min_d2(pts, v, f)
        d_all = np.sqrt(d2)
        d_last = np.sqrt(R.min_d2(pts, v, f[-1:]))
        d_rest = np.sqrt(R.min_d2(pts, v, f[:-1]))
        assert d_rest.min() > max(C.QUERY_DISTANCES) + C.GUARD and np.array_equal(d_all, d_last)
        for q in C.QUERY_DISTANCES:
            assert (np.abs(d_all - q) > C.GUARD).all()
            want = R.near_mask(pts, d2, q)
            assert want.any() and not want.all(), (F, k, q)
            assert np.array_equal(R.near_mask_f32(pts, v, f, q), want)
        near = d_all <= C.QUERY_DISTANCES[0]
        assert np.array_equal(np.nonzero(near)[0], np.arange(0, 65, 4) if k == 0 else [(0, 63)[k - 1]])


# ---- the C boundary ------------------------------------------------------------------------------

def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): (0 if m.group(2).strip() in ("", "void") else m.group(2).count(",") + 1)
            for m in re.finditer(r"\b(gsr_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}


def test_lib_declares_and_exports_the_header_entry_points():
    from diff_gaussian_rasterization import _lib
    decl = _declared()
    assert set(decl) == {"gsr_mesh_index_create", "gsr_mesh_index_destroy", "gsr_mesh_index_info",
                         "gsr_mesh_near_mask", "gsr_voxel_mean_scratch_bytes", "gsr_voxel_mean"}
    table = getattr(_lib, "LIDAR_SIGNATURES", {})
    assert set(table) == set(decl), "ctypes table out of sync with include/gsr_lidar.h"
    for name, n in decl.items():
        assert len(table[name][1]) == n, f"{name}: {len(table[name][1])} ctypes arguments, the header has {n}"
    others = (set(_lib.SIGNATURES) | set(_lib.GT_SIGNATURES) | set(_lib.EVAL_SIGNATURES)
              | set(_lib.HIER_BUILD_SIGNATURES) | set(_lib.HIER_MERGE_SIGNATURES) | set(_lib.LPIPS_SIGNATURES)
              | set(_lib.MODEL_INIT_SIGNATURES))
    assert not set(table) & others
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in decl:
        assert hasattr(raw, name), f"libgsr_hip.so does not export {name}"
    L = _lib.load()
    assert L.gsr_abi_version() == 7 == _lib.ABI_VERSION  # new entry points only
    assert L.gsr_mesh_index_create.restype is ctypes.c_void_p
    assert L.gsr_mesh_index_create.argtypes[4] is ctypes.c_double
    assert L.gsr_voxel_mean.argtypes[4] is ctypes.c_double
    assert L.gsr_voxel_mean_scratch_bytes.restype is ctypes.c_size_t


def test_calls_validate_without_gpu():
    """Argument checks and host arithmetic that come before any device work."""
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    assert not L.gsr_mesh_index_create(0, None, 0, None, 0.1, None)
    assert b"gsr_mesh_index_create" in L.gsr_last_error()
    assert not L.gsr_mesh_index_create(3, None, 1, None, 0.1, None)
    info = (ctypes.c_int64 * 9)()
    assert L.gsr_mesh_index_info(None, info, 9) != 0
    assert L.gsr_mesh_near_mask(4, None, None, 0.1, None, None, None) != 0
    assert L.gsr_mesh_near_mask(-1, None, None, 0.1, None, None, None) != 0
    L.gsr_mesh_index_destroy(None)
    assert L.gsr_voxel_mean_scratch_bytes(0) == 0 and L.gsr_voxel_mean_scratch_bytes(1 << 31) == 0
    prev = 0
    for n in (1, 64, 4099, 1 << 20, 20_000_000):
        b = L.gsr_voxel_mean_scratch_bytes(n)
        assert 24 * n <= b <= 40 * n + (1 << 22) and b >= prev, (n, b)
        prev = b
    n_out = ctypes.c_int64(-1)
    assert L.gsr_voxel_mean(4, None, None, None, 0.1, None, None, None, None, ctypes.byref(n_out), None) != 0
    assert L.gsr_voxel_mean(0, None, None, None, -1.0, None, None, None, None, ctypes.byref(n_out), None) != 0
    assert L.gsr_voxel_mean(0, None, None, None, 0.1, None, None, None, None, ctypes.byref(n_out), None) == 0
    assert n_out.value == 0


def test_wrappers_refuse_cpu_tensors():
    import torch
    from gs_train import lidar
    c = C.mesh_case("features")
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        lidar.MeshIndex(torch.from_numpy(c["vertices"]), torch.from_numpy(c["faces"]))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        lidar.voxel_downsample(torch.zeros(4, 3), None, 0.1)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        lidar.prepare_chunk_cloud(torch.zeros(4, 3), None, (0, 0, 0), (1, 1, 1))
    assert np.array_equal(lidar.crop_bounds((3.0, 2.0, 0.0), (4.0, 2.0, 9.0)), R.crop_bounds((3.0, 2.0), (4.0, 2.0)))


# ---- the PLY mesh reader -------------------------------------------------------------------------

def _header(fmt, elements):
    lines = ["ply", f"format {fmt} 1.0", "comment written by the test"]
    for name, count, props in elements:
        lines.append(f"element {name} {count}")
        lines += [f"property {p}" for p in props]
    return ("\n".join(lines) + "\nend_header\n").encode("ascii")


def _small_mesh():
    c = C.mesh_case("sizes_P64_F2")
    return c["vertices"], c["faces"]


@pytest.mark.parametrize("itype", ["int", "uint"])
def test_ply_mesh_binary(tmp_path, itype):
    from gs_train.lidar import read_ply_mesh
    v, f = _small_mesh()
    rows = np.zeros(len(v), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("q", "u1")]))
    rows["x"], rows["y"], rows["z"] = v[:, 0], v[:, 1], v[:, 2]
    faces = b"".join(bytes([3]) + struct.pack("<3i", *t) for t in f.tolist())
    p = tmp_path / "m.ply"
    p.write_bytes(_header("binary_little_endian",
                          [("vertex", len(v), ["float x", "float y", "float z", "uchar q"]),
                           ("face", len(f), [f"list uchar {itype} vertex_indices"])]) + rows.tobytes() + faces)
    rv, rf = read_ply_mesh(str(p))
    assert rv.dtype == np.float32 and rf.dtype == np.int32
    assert np.array_equal(rv, v) and np.array_equal(rf, f)


def test_ply_mesh_ascii_and_the_xyz_reader_still_reads_it(tmp_path):
    from gs_train.gtcloud import read_ply_xyz
    from gs_train.lidar import read_ply_mesh
    v, f = _small_mesh()
    body = "".join(f"{x!r} {y!r} {z!r}\n" for x, y, z in v.astype(np.float64).tolist())
    body += "".join(f"3 {a} {b} {c}\n" for a, b, c in f.tolist())
    p = tmp_path / "a.ply"
    p.write_bytes(_header("ascii", [("vertex", len(v), ["double x", "double y", "double z"]),
                                    ("face", len(f), ["list uchar int vertex_indices"])]) + body.encode("ascii"))
    rv, rf = read_ply_mesh(str(p))
    assert np.array_equal(rv, v) and np.array_equal(rf, f)
    assert np.array_equal(read_ply_xyz(str(p)), v)


def test_ply_mesh_rejects_what_it_does_not_read(tmp_path):
    from gs_train.lidar import read_ply_mesh
    v, f = _small_mesh()
    vb = v.astype("<f4").tobytes()
    vert = ("vertex", len(v), ["float x", "float y", "float z"])
    tri = b"".join(bytes([3]) + struct.pack("<3i", *t) for t in f.tolist())
    files = {
        "nofaces": _header("binary_little_endian", [vert]) + vb,
        "quad": _header("binary_little_endian", [vert, ("face", 1, ["list uchar int vertex_indices"])]) + vb
                + bytes([4]) + struct.pack("<4i", 0, 1, 2, 3),
        "short": _header("binary_little_endian", [vert, ("face", len(f), ["list uchar int vertex_indices"])]) + vb
                 + tri[:-2],
        "listtype": _header("binary_little_endian", [vert, ("face", len(f), ["list int int vertex_indices"])]) + vb + tri,
        "extra": _header("binary_little_endian", [vert, ("face", len(f), ["list uchar int vertex_indices", "uchar flag"])])
                 + vb + tri,
        "range": _header("binary_little_endian", [vert, ("face", 1, ["list uchar int vertex_indices"])]) + vb
                 + bytes([3]) + struct.pack("<3i", 0, 1, len(v)),
        "asciiquad": _header("ascii", [("vertex", 3, ["float x", "float y", "float z"]),
                                       ("face", 2, ["list uchar int vertex_indices"])])
                     + b"0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n4 0 1 2 0\n",
        "big": _header("binary_big_endian", [vert, ("face", len(f), ["list uchar int vertex_indices"])]) + vb + tri,
    }
    for name, data in files.items():
        p = tmp_path / (name + ".ply")
        p.write_bytes(data)
        with pytest.raises(ValueError):
            read_ply_mesh(str(p))
