"""CPU tests of the ground-truth cloud constraint (gs_train.gtcloud, include/gsr_gtcloud.h): the PLY
reader, the reference-generated fixtures against the d2 rule of tests/gt_ref.py, and the ctypes
table against the header."""
from __future__ import annotations

import ctypes
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gt_ref  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
HEADER = os.path.join(REPO, "include", "gsr_gtcloud.h")


# ---- the PLY reader ---------------------------------------------------------------------------

def _header(fmt, elements):
    lines = ["ply", f"format {fmt} 1.0", "comment written by the test"]
    for name, count, props in elements:
        lines.append(f"element {name} {count}")
        lines += [f"property {p}" for p in props]
    return ("\n".join(lines) + "\nend_header\n").encode("ascii")


def _points(n=7, seed=0):
    return (np.random.default_rng(seed).normal(size=(n, 3)) * 30).astype(np.float32)


def test_ply_ascii_float_with_extra_properties(tmp_path):
    from gs_train.gtcloud import read_ply_xyz
    p = _points()
    body = "".join(f"{i} {x!r} {y!r} {z!r} 255\n" for i, (x, y, z) in enumerate(p.astype(np.float64).tolist()))
    body += "3 0 1 2\n"
    f = tmp_path / "a.ply"
    f.write_bytes(_header("ascii", [("vertex", len(p), ["int id", "float x", "float y", "float z", "uchar red"]),
                                    ("face", 1, ["list uchar int vertex_indices"])]) + body.encode("ascii"))
    out = read_ply_xyz(str(f))
    assert out.dtype == np.float32 and out.flags.c_contiguous
    assert np.array_equal(out, p)


@pytest.mark.parametrize("ctype,fmt", [("float", "<f4"), ("double", "<f8")])
def test_ply_binary_little_endian(tmp_path, ctype, fmt):
    from gs_train.gtcloud import read_ply_xyz
    p = _points(11, seed=1)
    # properties out of order and an element before the vertices
    dt = np.dtype([("z", fmt), ("intensity", "<u2"), ("x", fmt), ("y", fmt)])
    rows = np.zeros(len(p), dt)
    rows["x"], rows["y"], rows["z"], rows["intensity"] = p[:, 0], p[:, 1], p[:, 2], 7
    pre = struct.pack("<2i", 5, 6)
    f = tmp_path / "b.ply"
    f.write_bytes(_header("binary_little_endian",
                          [("sensor", 2, ["int serial"]),
                           ("vertex", len(p), [f"{ctype} z", "ushort intensity", f"{ctype} x", f"{ctype} y"]),
                           ("face", 1, ["list uchar int vertex_indices"])])
                  + pre + rows.tobytes() + bytes([3]) + struct.pack("<3i", 0, 1, 2))
    assert np.array_equal(read_ply_xyz(str(f)), p)


def test_ply_rejects_what_it_does_not_read(tmp_path):
    from gs_train.gtcloud import read_ply_xyz
    p = _points(3)
    big = tmp_path / "big.ply"
    big.write_bytes(_header("binary_big_endian", [("vertex", 3, ["float x", "float y", "float z"])])
                    + p.astype(">f4").tobytes())
    faces = tmp_path / "faces.ply"
    faces.write_bytes(_header("ascii", [("face", 1, ["list uchar int vertex_indices"])]) + b"3 0 1 2\n")
    noz = tmp_path / "noz.ply"
    noz.write_bytes(_header("ascii", [("vertex", 1, ["float x", "float y"])]) + b"1 2\n")
    ints = tmp_path / "ints.ply"
    ints.write_bytes(_header("ascii", [("vertex", 1, ["int x", "int y", "int z"])]) + b"1 2 3\n")
    short = tmp_path / "short.ply"
    short.write_bytes(_header("binary_little_endian", [("vertex", 3, ["float x", "float y", "float z"])])
                      + p.tobytes()[:-4])
    notply = tmp_path / "not.ply"
    notply.write_bytes(b"solid stl\n")
    for f in (big, faces, noz, ints, short, notply):
        with pytest.raises(ValueError):
            read_ply_xyz(str(f))


# ---- the fixtures against the rule ------------------------------------------------------------

@pytest.mark.parametrize("case", ["plain", "scaffold"])
def test_fixture_agrees_with_the_d2_rule(case):
    """What the reference's compare_points_to_gt returned on the fixture's own rows is what
    tests/gt_ref.py decides, the bounds are load_gt_point_cloud's, the counts are the mask's, and
    the rows densify_and_prune left are the rows the mask keeps."""
    g = np.load(os.path.join(GOLD, f"densify_prune_gt_{case}.npz"))
    cloud, thr = g["cloud"], float(g["threshold"])
    assert cloud.shape == (4000, 3) and cloud.dtype == np.float32
    assert np.array_equal(g["bounds"], np.array(gt_ref.bounds(cloud), np.float32))
    xyz, existing, protected, mask = g["cmp_xyz"], g["cmp_existing"], g["cmp_protected"], g["cmp_mask"]
    assert np.array_equal(gt_ref.compare_points_to_gt(xyz, cloud, thr, existing, protected), mask)
    dist = mask & ~existing
    scaffold = int(g["scaffold"])
    assert int(g["gt_pruned"]) == int(dist.sum()) > 0
    assert int(g["gt_pruned_fixed"]) == int(dist[:scaffold].sum())
    assert (int(g["gt_pruned_fixed"]) > 0) == (case == "scaffold")
    assert not existing[:scaffold].any()
    assert np.array_equal(g["out_xyz"], xyz[~mask])
    # the fixture exercises every branch of the rule
    inside = gt_ref.inside_bounds(xyz, cloud)
    far = gt_ref.far_mask(xyz, cloud, thr)  # D without the skips
    assert (protected & far).any() and (existing & far).any()
    assert (~inside & ~mask).any() and (gt_ref.min_d2(xyz[~inside], cloud) > thr * thr).any()


# ---- the bindings against the header ----------------------------------------------------------

def _declarations():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(gsr_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out


def test_lib_declares_the_header_entry_points():
    from diff_gaussian_rasterization import _lib
    decl = _declarations()
    assert set(decl) == {"gsr_gt_index_create", "gsr_gt_index_destroy", "gsr_gt_index_bounds", "gsr_gt_index_info",
                         "gsr_gt_far_mask", "gsr_densify_plan_gt"}
    table = getattr(_lib, "GT_SIGNATURES", {})
    assert set(table) == set(decl), "ctypes table out of sync with include/gsr_gtcloud.h"
    for name, n in decl.items():
        assert len(table[name][1]) == n, f"{name}: {len(table[name][1])} ctypes arguments, the header has {n}"
    assert not set(table) & set(_lib.SIGNATURES)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in decl:
        assert hasattr(lib, name), f"libgsr_hip.so does not export {name}"
    L = _lib.load()
    assert L.gsr_gt_index_create.restype is ctypes.c_void_p
    assert L.gsr_densify_plan_gt.argtypes[11] is ctypes.c_double


def test_index_calls_validate_without_gpu():
    """Argument checks return before any device work."""
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    assert not L.gsr_gt_index_create(0, None, 0.05, None)
    assert b"gsr_gt_index_create" in L.gsr_last_error()
    b = (ctypes.c_float * 4)()
    assert L.gsr_gt_index_bounds(None, b) != 0
    assert L.gsr_gt_far_mask(4, None, None, 0.05, None, None, None) != 0
    L.gsr_gt_index_destroy(None)
