"""CPU tests of the mesh ray cast and depth encode references (tests/mesh_depth_ref.py), the cases
(tests/mesh_depth_cases.py) and the host side of gs_train/mesh_depth.py: the float64 ray cast against an
independent intersection algorithm, analytic planes and spheres and dense sampling; the float64 encode
against the reference-generated tests/golden/depth_encode.npz; the PNG and JSON files; the conditions
the GPU test's comparison rests on; and the float32 restatement's distance from float64 in error
scales, written to profiles/r20_mesh_depth_margins.jsonl (the GPU test's bar is 4x it)."""
from __future__ import annotations

import ctypes
import json
import os
import re
import struct
import zlib

import numpy as np
import pytest

import mesh_depth_cases as C
import mesh_depth_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "depth_encode.npz")
MARGINS = os.path.join(REPO, "profiles", "r20_mesh_depth_margins.jsonl")
BOUNDARY_CAP = 0.15


# ---- the float64 ray cast against independent checks -------------------------------------------------

def _moller_trumbore(vertices, faces, cam, W, H):
    """Nearest ray distance per pixel by the Moller-Trumbore barycentric solve (two-sided), float64."""
    Rm, Cc, *_ = R.camera64(cam)
    f = R._valid_faces(vertices, faces)
    tri = (np.asarray(vertices, np.float64)[f] - Cc) @ Rm.T
    dx, dy = R.rays(cam, W, H)
    d = np.stack([dx, dy, np.ones_like(dx)], 1)
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    best = np.full(len(d), np.inf)
    for s0 in range(0, len(tri), 256):
        a, e1, e2 = tri[s0:s0 + 256, 0], tri[s0:s0 + 256, 1] - tri[s0:s0 + 256, 0], tri[s0:s0 + 256, 2] - tri[s0:s0 + 256, 0]
        h = np.cross(dn[:, None, :], e2[None])
        det = (e1[None] * h).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (-a[None] * h).sum(-1) / det
            q = np.cross(-a, e1)
            v = (dn[:, None, :] * q[None]).sum(-1) / det
            t = (e2 * q).sum(-1)[None] / det
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
        best = np.minimum(best, np.where(ok, t, np.inf).min(1))
    return np.where(np.isfinite(best), best, 0.0).reshape(H, W)


@pytest.mark.parametrize("name", ["64x48_F600_K3", "shifted_2000m", "fx_ne_fy_off_centre", "icosphere_from_inside",
                                  "oversize_frame_filling", "crossing_camera_plane", "crossing_from_the_side"])
def test_float64_cast_against_another_intersection_algorithm(name):
    c = C.by_name(name)
    for cam, r in zip(c["cams"], C.reference(name)):
        other = _moller_trumbore(c["vertices"], c["faces"], cam, c["W"], c["H"])
        dec = ~r["boundary"]
        assert np.array_equal((other > 0)[dec], (r["distance"] > 0)[dec])
        scale = np.abs(c["vertices"]).max() + 1
        assert np.abs(other - r["distance"])[dec].max() <= 1e-9 * scale


def test_float64_cast_on_an_analytic_plane_and_sphere():
    # the plane n . x = h seen from the origin: distance h / (n . d^)
    n = np.array([0.2, -0.1, 1.0])
    n /= np.linalg.norm(n)
    h = 7.0
    u, v = np.cross(n, [1.0, 0, 0]), None
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    p0 = n * h
    vert = np.array([p0 - 90 * u - 70 * v, p0 + 90 * u - 70 * v, p0 + 100 * v], np.float32)
    cam = C.axis_cam(40, 30, 20.5, 17.0)
    r = R.cast64(vert, [[0, 1, 2]], cam, 48, 36)
    dx, dy = R.rays(cam, 48, 36)
    d = np.stack([dx, dy, np.ones_like(dx)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tv = vert.astype(np.float64)
    nn = np.cross(tv[1] - tv[0], tv[2] - tv[0])  # the float32 vertices' own plane
    want = ((nn @ tv[0]) / (d @ nn)).reshape(36, 48)
    assert (r["distance"] > 0).all() and not r["boundary"].any()
    assert np.abs(r["distance"] - want).max() < 1e-12 * h
    z = R.cast64(vert, [[0, 1, 2]], cam, 48, 36, mode=1)["distance"]
    assert np.abs(z - want * d[:, 2].reshape(36, 48)).max() < 1e-12 * h
    # a sphere of radius r around the camera: every ray hits between the inscribed radius and r
    sv, sf = C.icosphere(3, 5.0)
    rr = R.cast64(sv, sf, C.look_at((0, 0, 0), (1, 0.3, 0.2), 12, 12, 16, 12), 32, 24)
    t = sv[sf].astype(np.float64)
    pn = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    inscribed = np.abs((pn * t[:, 0]).sum(1) / np.linalg.norm(pn, axis=1)).min()
    assert (rr["distance"] >= inscribed - 1e-6).all() and (rr["distance"] <= 5.0 + 1e-6).all()
    assert 4.9 < inscribed < 5.0


def test_float64_cast_against_dense_barycentric_sampling():
    """Every sample of a triangle that projects (almost) onto a pixel centre is at least as far as the
    pixel's distance, and every hit pixel has such a sample at its distance."""
    c = C.by_name("64x48_F600_K3")
    cam, r = c["cams"][1], C.reference(c["name"])[1]
    Rm, Cc, fx, fy, cx, cy = R.camera64(cam)
    tri = (c["vertices"].astype(np.float64)[c["faces"]] - Cc) @ Rm.T
    n = 96
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1))
    keep = (i + j) <= n
    w = np.stack([i[keep], j[keep], n - i[keep] - j[keep]], 1) / n  # (S, 3)
    pts = np.einsum("sk,fkc->fsc", w, tri).reshape(-1, 3)
    nrm = np.repeat(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), len(w), axis=0)
    cos = np.abs((nrm * pts).sum(1)) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(pts, axis=1))
    nrm, cos = None, cos[pts[:, 2] > 0]
    pts = pts[pts[:, 2] > 0]
    px, py = fx * pts[:, 0] / pts[:, 2] + cx - 0.5, fy * pts[:, 1] / pts[:, 2] + cy - 0.5
    ix, iy = np.rint(px).astype(int), np.rint(py).astype(int)
    tol = 0.02
    m = (np.abs(px - ix) < tol) & (np.abs(py - iy) < tol) & (ix >= 0) & (ix < c["W"]) & (iy >= 0) & (iy < c["H"])
    dist = np.linalg.norm(pts[m], axis=1)
    got = r["distance"][iy[m], ix[m]]
    dec = ~r["boundary"][iy[m], ix[m]]
    # a sample tol pixels off the centre on each axis lies on a ray sqrt(2) tol / f off; along the surface
    # the distance changes by at most distance x angle x tan(incidence) <= distance x angle / cos, with
    # the steepest incidence any sample is seen under
    steep = cos[m].min()
    assert steep > 0.1
    slack = 2 * tol / min(fx, fy) * dist / steep
    assert m.sum() > 2000
    assert ((got > 0) | ~dec).all()
    assert (got[dec] <= dist[dec] + slack[dec]).all()
    nearest = np.full((c["H"], c["W"]), np.inf)
    np.minimum.at(nearest, (iy[m], ix[m]), dist - got)
    seen = np.isfinite(nearest) & ~r["boundary"]
    assert seen.sum() > 500 and (np.abs(nearest[seen]) <= (2.5 * tol / min(fx, fy) / steep * r["distance"])[seen]).all()


# ---- the conditions the GPU comparison rests on ------------------------------------------------------

def test_cases_meet_their_conditions():
    for c in C.all_cases():
        refs = C.reference(c["name"])
        assert len(refs) == len(c["cams"])
        for k, r in enumerate(refs):
            frac = r["boundary"].mean()
            if not c["fan"] and not c["exact"]:
                assert frac <= BOUNDARY_CAP, (c["name"], k, frac)
            assert set(r["cands"]) == set(np.nonzero(r["boundary"].reshape(-1))[0].tolist())
            if c["closed"] is not None:
                cl = c["closed"][k]
                assert (r["distance"][cl] > 0).all(), (c["name"], k)  # the float64 rule finds no hole
                for p, (cd, _) in r["cands"].items():
                    if cl[p // c["W"], p % c["W"]]:
                        assert (cd > 0).any(), (c["name"], k, p)  # something to hit: 0 is no candidate there
            if c["zero"]:
                assert (r["distance"] == 0).all()
            for (kk, iy, ix, val) in c["exact"]:
                if kk == k:
                    assert r["distance"][iy, ix] == val, (c["name"], r["distance"][iy, ix], val)


def test_cases_cover_what_they_claim():
    names = set(C.NAMES)
    sizes = {(c["W"], c["H"]) for c in C.all_cases()}
    assert {(1, 1), (16, 16), (17, 15), (64, 48), (130, 70)} <= sizes
    assert {1, 3, 65} <= {len(c["cams"]) for c in C.all_cases()}
    assert {1, 2, 4097} <= {len(c["faces"]) for c in C.all_cases()}
    assert {0, 1} == {c["mode"] for c in C.all_cases()}
    # oversize: the frame-filling triangle's bounds cover every tile, more than max(4, T / 2)
    c = C.by_name("oversize_frame_filling")
    assert (C.reference(c["name"])[0]["distance"] > 0).all() and 12 > max(4, 12 // 2)
    # the fan: more than one LDS batch of 256 in one tile, nothing outside it
    c = C.by_name("fan_5000_in_one_tile")
    hit = C.reference(c["name"])[0]["distance"] > 0
    assert len(c["faces"]) == 5000 and hit[16:, 16:].any() and not hit[:16].any() and not hit[:, :16].any()
    # crossing: vertices on both sides of the camera plane, and the triangle is seen
    for nm in ("crossing_camera_plane", "crossing_from_the_side"):
        c = C.by_name(nm)
        z = c["vertices"][:, 2]
        assert z.min() < 0 < z.max() and (C.reference(nm)[0]["distance"] > 0).any()
    # the sub-pixel triangles: one hits exactly one pixel, the other none
    r = C.reference("subpixel_triangles")[0]
    assert (r["distance"] > 0).sum() == 1 and r["distance"][5, 9] > 0 and not r["boundary"].any()
    # layers: the nearer plane wins where both cover, by 1e-3 against an error scale of 1e-6
    r = C.reference("layers_1mm_apart")[0]
    assert (r["scale"][r["distance"] > 0] < 1e-5).all()
    # the shifted scene is the unshifted one
    a, b = C.reference("64x48_F600_K3")[0], C.reference("shifted_2000m")[0]
    assert np.array_equal(a["distance"] > 0, b["distance"] > 0)
    assert np.abs(a["distance"] - b["distance"]).max() < 2e-3  # the float32 vertices moved by up to 2^-14 m
    # bad faces are skipped: the case equals its good part
    c = C.by_name("non_finite_and_out_of_range")
    good = R.cast64(c["vertices"][:25], c["faces"][:32], c["cams"][0], 16, 16)
    assert np.array_equal(good["distance"], C.reference(c["name"])[0]["distance"])
    # the diagonal passes exactly through pixel centres: both triangles' shared edge function is 0 there
    c = C.by_name("quad_diagonal_through_centres")
    r = C.reference(c["name"])[0]
    assert r["boundary"][np.arange(16), np.arange(16)][c["closed"][0][np.arange(16), np.arange(16)]].all()
    assert {"tfar_exact_hit", "tfar_one_above_miss", "tnear_exact_miss", "tnear_one_above_hit", "wholly_behind",
            "outside_each_side", "zero_area_and_collinear", "coincident_triangles", "principal_point_outside",
            "icosphere_from_inside"} <= names
    enc = {n for n, _, _ in C.encode_cases()}
    assert {"code_limits", "min_and_max_depth", "all_background", "one_valid_pixel", "two_equal_valid_pixels",
            "one_pixel_map", "130x70", "K65"} <= enc


def test_float32_restatement_margin_is_recorded():
    """The float32 restatement (the kernel's arithmetic, all pairs) decides every decided pixel as
    float64 does, meets the exact values, leaves the zero cases zero and closed surfaces closed; its
    largest distance from float64 in error scales goes to profiles/r20_mesh_depth_margins.jsonl."""
    worst, rows = (0.0, ""), []
    for c in C.all_cases():
        case_worst = 0.0
        for k, (cam, r) in enumerate(zip(c["cams"], C.reference(c["name"]))):
            if k >= 5 and len(c["cams"]) > 5 and k % 16:
                continue  # every sixteenth of the ring of 65
            d32 = R.cast32(c["vertices"], c["faces"], cam, c["W"], c["H"], c["tnear"], c["tfar"], c["mode"])
            m, same = R.margin_units(d32, r)
            assert same, (c["name"], k)
            case_worst = max(case_worst, m)
            if c["zero"]:
                assert (d32 == 0).all(), c["name"]
            if c["closed"] is not None:
                assert (d32[c["closed"][k]] > 0).all(), c["name"]
            for (kk, iy, ix, val) in c["exact"]:
                if kk == k:
                    assert d32[iy, ix] == np.float32(val), (c["name"], d32[iy, ix], val)
            assert not R.judge(d32, r, 4 * max(m, 1.0), None if c["closed"] is None else c["closed"][k])
        rows.append({"kind": "cpu_f32", "case": c["name"], "units": case_worst})
        if case_worst >= worst[0]:
            worst = (case_worst, c["name"])
    assert 0.5 < worst[0] < 16, worst  # a bar of dozens of error scales would hold nothing
    kept = []
    if os.path.exists(MARGINS):
        with open(MARGINS) as f:
            kept = [ln for ln in f if ln.strip() and json.loads(ln).get("kind") not in ("cpu_f32", "cpu_f32_worst")]
    os.makedirs(os.path.dirname(MARGINS), exist_ok=True)
    with open(MARGINS, "w") as f:
        f.write(json.dumps({"kind": "cpu_f32_worst", "case": worst[1], "units": worst[0]}) + "\n")
        for row in rows:
            f.write(json.dumps(row) + "\n")
        f.writelines(kept)


# ---- the encode --------------------------------------------------------------------------------------

def test_float64_encode_equals_the_reference_fixture():
    g = np.load(GOLD)
    assert int(g["n"]) >= 8
    wrapped = False
    for k in range(int(g["n"])):
        depth, bg = R.depth_of_mm(g[f"mm_{k}"])
        assert np.array_equal(depth, g[f"depth_{k}"]) and np.array_equal(bg, g[f"background_{k}"]), k
        wrapped |= bool(((g[f"mm_{k}"] == 65536.0) & (depth == 0) & ~bg).any())
        for s, (lo, hi) in enumerate(g["settings"]):
            u16, scale, offset = R.normalise64(depth, bg, lo, None if hi < 0 else hi)
            assert np.array_equal(u16, g[f"u16_{k}_{s}"]), (k, s)
            assert (scale, offset) == tuple(g[f"scale_offset_{k}_{s}"]), (k, s)
    assert wrapped  # 65536 mm exactly: units = 16384 leaves the unit bits; the decode gives 0, not background


def test_encode_cases_are_what_they_claim():
    by = {n: (d, kw) for n, d, kw in C.encode_cases()}
    d, _ = by["code_limits"]
    mm = 1000.0 * d.astype(np.float64)
    for lim in (1.0, 65536.0, 262144.0, 1048576.0):  # the float32 nearest each limit and one on either side
        assert (mm < lim).any() and (mm > lim).any() and np.nanmin(np.abs(mm - lim)) <= lim * 2.0 ** -23
    u16, scale, offset = R.encode64(*by["all_background"][:1])
    assert not u16.any() and not scale.any() and not offset.any()
    u16, scale, offset = R.encode64(by["one_valid_pixel"][0])
    assert not u16.any() and scale[0] == 0 and offset[0] == 1 / 7.3  # 7300 mm is a multiple of the 4 mm step
    u16, scale, offset = R.encode64(by["two_equal_valid_pixels"][0])
    assert not u16.any() and scale[0] == 0 and offset[0] > 0
    d, kw = by["min_and_max_depth"]
    u16, scale, offset = R.encode64(d, **kw)
    depth, _ = R.depth_of(d[0], True)
    assert 1 / offset[0] == depth[(depth > 0.1) & (depth < 50.0)].max()
    u16, scale, offset = R.encode64(by["K65"][0])
    assert scale[7] == 0 and offset[7] == 0 and scale[9] == 0 and offset[9] == 0.25 and (scale[:7] > 0).all()
    assert u16.max() == 65535 and by["130x70"][0].shape == (2, 70, 130)


# ---- the files ---------------------------------------------------------------------------------------

def _chunks(raw):
    pos, out = 8, []
    while pos < len(raw):
        (n,) = struct.unpack(">I", raw[pos:pos + 4])
        out.append((raw[pos + 4:pos + 8], raw[pos + 8:pos + 8 + n], struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0]))
        pos += 12 + n
    return out


def test_png16_round_trip_and_crcs(tmp_path):
    from gs_train import mesh_depth as M
    rng = np.random.default_rng(5)
    for shape in ((1, 1), (3, 7), (70, 130)):
        img = rng.integers(0, 65536, shape).astype(np.uint16)
        img.flat[0], img.flat[-1] = 0, 65535
        p = tmp_path / f"{shape[0]}x{shape[1]}.png"
        M.save_png16(p, img)
        assert np.array_equal(M.load_png16(p), img)
        raw = p.read_bytes()
        assert raw[:8] == b"\x89PNG\r\n\x1a\n"
        ch = _chunks(raw)
        assert [c[0] for c in ch] == [b"IHDR", b"IDAT", b"IEND"]
        for kind, data, crc in ch:
            assert crc == (zlib.crc32(kind + data) & 0xFFFFFFFF)
        assert struct.unpack(">IIBBBBB", ch[0][1]) == (shape[1], shape[0], 16, 0, 0, 0, 0)
    # a file another writer made: every row filter, several IDAT chunks
    img = (np.arange(5 * 9).reshape(5, 9) * 1431 % 65536).astype(np.uint16)
    be = img.astype(">u2").view(np.uint8).reshape(5, 18).astype(np.int32)
    rows, prev = [], np.zeros(18, np.int32)
    for y, ft in enumerate((0, 1, 2, 3, 4)):
        left = np.concatenate([np.zeros(2, np.int32), be[y, :-2]])
        ul = np.concatenate([np.zeros(2, np.int32), prev[:-2]])
        pa, pb, pc = np.abs(prev - ul), np.abs(left - ul), np.abs(left + prev - 2 * ul)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
        pred = (np.zeros(18, np.int32), left, prev, (left + prev) // 2, paeth)[ft]
        rows.append(bytes([ft]) + ((be[y] - pred) % 256).astype(np.uint8).tobytes())
        prev = be[y]
    z = zlib.compress(b"".join(rows))
    chunk = lambda kind, data: struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    raw = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 9, 5, 16, 0, 0, 0, 0)) + \
        chunk(b"tEXt", b"k\x00v") + chunk(b"IDAT", z[:7]) + chunk(b"IDAT", z[7:]) + chunk(b"IEND", b"")
    p = tmp_path / "filters.png"
    p.write_bytes(raw)
    assert np.array_equal(M.load_png16(p), img)
    bad = bytearray(raw)
    bad[40] ^= 1
    (tmp_path / "bad.png").write_bytes(bytes(bad))
    with pytest.raises(ValueError):
        M.load_png16(tmp_path / "bad.png")
    with pytest.raises(ValueError):
        M.save_png16(tmp_path / "x.png", np.zeros((2, 2), np.uint8))


def test_depth_params_round_trip(tmp_path):
    from gs_train import mesh_depth as M
    names = ["cam1/00002_B_b1.jpg", "cam0/00001_A_f1.jpg", "cam0/00003_C_l1.jpg", "cam2/none.jpg"]
    maps = {"cam0/00001_A_f1": (0.25, 0.01), "cam1/00002_B_b1": (0.0, 0.5), "cam0/00003_C_l1": (0.75, 0.002)}
    p = tmp_path / "depth_params.json"
    assert M.write_depth_params(p, names, maps, default_scale=0.0, default_offset=0.0) == 4
    text = p.read_text()
    want = {"cam0/00001_A_f1": {"scale": 0.25, "offset": 0.01}, "cam0/00003_C_l1": {"scale": 0.75, "offset": 0.002},
            "cam1/00002_B_b1": {"scale": 0.0, "offset": 0.5}, "cam2/none": {"scale": 0.0, "offset": 0.0}}
    assert text == json.dumps(want, indent=4)  # sorted keys without extension, indent 4
    got = M.read_depth_params(p)
    assert list(got) == sorted(got) and all(got[k]["med_scale"] == 0.5 for k in got)
    assert {k: {"scale": v["scale"], "offset": v["offset"]} for k, v in got.items()} == want
    M.write_depth_params(p, names[:1], {})
    assert M.read_depth_params(p)["cam1/00002_B_b1"] == {"scale": 0.0, "offset": 0.0, "med_scale": 0}
    # float64 values survive the file exactly
    x = {"a": (1 / 3, 2.0 ** -40 + 1e-9)}
    M.write_depth_params(p, ["a.png"], x)
    r = M.read_depth_params(p)["a"]
    assert (r["scale"], r["offset"]) == x["a"]


# ---- the C ABI and the wrappers without a GPU ---------------------------------------------------------

def test_lib_declares_and_exports_the_header_entry_points():
    from diff_gaussian_rasterization import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "gsr_mesh_depth.h")).read(), flags=re.S)
    decl = {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\b(gsr_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}
    assert set(decl) == {"gsr_mesh_distance_scratch_bytes", "gsr_mesh_distance_maps", "gsr_depth_encode_scratch_bytes",
                         "gsr_depth_encode"}
    table = _lib.MESH_DEPTH_SIGNATURES
    assert set(table) == set(decl)
    for name, n in decl.items():
        assert len(table[name][1]) == n, name
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in decl:
        assert hasattr(raw, name)
    assert _lib.load().gsr_abi_version() == _lib.ABI_VERSION == 7  # new entry points only


def test_calls_validate_without_gpu():
    from diff_gaussian_rasterization import _lib
    L = _lib.load()
    assert L.gsr_mesh_distance_scratch_bytes(0, 5) == 0 and L.gsr_mesh_distance_scratch_bytes(1 << 20, 1 << 20) == 0
    assert L.gsr_mesh_distance_scratch_bytes(3, 100) >= 3 * 100 * 8
    args = lambda **kw: [kw.get(k, d) for k, d in (("V", 3), ("v", None), ("F", 1), ("f", None), ("K", 1), ("c", None),
                                                   ("W", 4), ("H", 4), ("tnear", 0.0), ("tfar", 10.0), ("mode", 0),
                                                   ("s", None), ("o", None), ("st", None), ("stream", None))]
    for kw in (dict(K=-1), dict(W=-1), dict(W=40000), dict(mode=2), dict(tnear=-1.0), dict(tfar=0.0), dict(tfar=float("inf")),
               dict(tnear=float("nan")), dict()):  # the last: NULL pointers
        assert L.gsr_mesh_distance_maps(*args(**kw)) != 0, kw
        assert b"gsr_mesh_distance_maps" in L.gsr_last_error()
    for kw in (dict(K=0), dict(W=0), dict(H=0)):  # no-ops
        assert L.gsr_mesh_distance_maps(*args(**kw)) == 0, kw
    assert L.gsr_depth_encode_scratch_bytes(0) == 0 and L.gsr_depth_encode_scratch_bytes(65) >= 65 * 32
    assert L.gsr_depth_encode(0, 4, 4, None, 1, 0.1, 0.0, None, None, None, None, None) == 0
    assert L.gsr_depth_encode(2, 0, 4, None, 1, 0.1, 0.0, None, None, None, None, None) == 0
    assert L.gsr_depth_encode(-1, 4, 4, None, 1, 0.1, 0.0, None, None, None, None, None) != 0
    assert L.gsr_depth_encode(1, 4, 4, None, 1, -0.1, 0.0, None, None, None, None, None) != 0
    assert L.gsr_depth_encode(1, 4, 4, None, 1, 0.1, 0.0, None, None, None, None, None) != 0  # NULL pointers


def test_wrappers_check_their_arguments_without_gpu():
    import torch
    from gs_train import mesh_depth as M
    c = C.by_name("16x16_F2_K3")
    q, t, k = c["cams"][:, :4], c["cams"][:, 4:7], c["cams"][:, 7:]
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        M.render_mesh_distance(torch.from_numpy(c["vertices"]), torch.from_numpy(c["faces"]), q, t, k, 16, 16)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        M.encode_depth_maps(torch.zeros(1, 4, 4))
    for bad in (dict(depth="w"), dict(tnear=-1.0), dict(tfar=0.0), dict(W=-1)):
        kw = dict(W=16, H=16)
        kw.update(bad)
        with pytest.raises(ValueError):
            M.render_mesh_distance(c["vertices"], c["faces"], q, t, k, **kw)
    with pytest.raises(ValueError):
        M._camera_table(q[:, :3], t, k)
    with pytest.raises(ValueError):
        M._camera_table(q, t[:2], k)
    with pytest.raises(ValueError):
        M._camera_table(q, t, k[:, :3])
    assert np.array_equal(M._camera_table(q, t, k[0]), np.concatenate([q, t, np.tile(k[0], (3, 1))], 1))
    # invdepth / depth_mask are cameras.py:72-74 on the stored map
    u16 = torch.tensor([[[0, 1, 65535], [32768, 7, 9]], [[1, 2, 3], [4, 5, 6]]], dtype=torch.int32)
    maps = M.DepthMaps(u16, np.array([0.5, 0.0]), np.array([0.125, 0.3]))
    inv = maps.invdepth()
    assert inv[1] is None and maps.depth_mask()[1] is None and inv[0].shape == (1, 2, 3)
    want = (u16[0].numpy().astype(np.float32) / np.float32(65536.0)) * np.float32(0.5) + np.float32(0.125)
    assert np.array_equal(inv[0][0].numpy(), want) and maps.depth_mask()[0].all()
