"""GPU tests of the mesh ray cast and the depth encode (include/gsr_mesh_depth.h, gs_train/mesh_depth.py)
against the float64 references of tests/mesh_depth_ref.py on the cases of tests/mesh_depth_cases.py.

Ray cast.  On decided pixels hit / miss equals float64 and the distance is within the bar; on boundary
pixels (an edge function within rounding of zero) the value is within the bar of one of the pixel's
candidates and never behind a decided hit; closed surfaces have no 0; the exact tfar / tnear ties come
out exactly; reruns and per-camera calls are bitwise equal.  The bar is 4x the float32 restatement's
own largest distance from float64 (profiles/r20_mesh_depth_margins.jsonl, kind cpu_f32_worst, measured
by tests/test_mesh_depth_cpu.py: the reference's error, not the kernel's) times the pixel's error scale,
4x for the kernel's freedom in operation order -- the convention of r12 and r17.

Encode.  u16, scale and offset equal the float64 encode exactly on authored distance maps.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np
import pytest
import torch

import mesh_depth_cases as C
import mesh_depth_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = os.path.join(REPO, "profiles", "r20_mesh_depth_margins.jsonl")


@functools.lru_cache(maxsize=None)
def bar_units():
    with open(MARGINS) as f:
        rows = [json.loads(ln) for ln in f if ln.strip()]
    worst = [r["units"] for r in rows if r.get("kind") == "cpu_f32_worst"]
    assert len(worst) == 1 and 0.5 < worst[0] < 16
    return 4.0 * worst[0]


def _render(c, cams=None, **kw):
    from gs_train import mesh_depth as M
    cams = c["cams"] if cams is None else cams
    args = dict(tnear=c["tnear"], tfar=c["tfar"], depth="z" if c["mode"] else "ray")
    args.update(kw)
    out = M.render_mesh_distance(c["vertices"], c["faces"], cams[:, :4], cams[:, 4:7], cams[:, 7:], c["W"], c["H"], **args)
    assert out.shape == (len(cams), c["H"], c["W"]) and out.dtype == torch.float32 and out.is_cuda
    return out


@pytest.mark.parametrize("name", C.NAMES)
def test_ray_cast_against_float64(name):
    c = C.by_name(name)
    got = _render(c).cpu().numpy()
    again = _render(c).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "reruns differ"
    assert np.isfinite(got).all() and (got >= 0).all()
    worst = 0.0
    for k, r in enumerate(C.reference(name)):
        closed = None if c["closed"] is None else c["closed"][k]
        m, _ = R.margin_units(got[k], r)
        worst = max(worst, m)
        bad = R.judge(got[k], r, bar_units(), closed)
        assert not bad, (name, k, bad[:3])
    print(f"{name}: kernel at most {worst:.3f} error scales from float64 on decided pixels (bar {bar_units():.3f})")
    if c["zero"]:
        assert not got.any()
    for (k, iy, ix, val) in c["exact"]:
        assert got[k, iy, ix] == np.float32(val), (name, got[k, iy, ix], val)


def test_batch_equals_single_camera_calls_bitwise():
    c = C.by_name("17x15_F2_K65")
    batch = _render(c)
    single = torch.cat([_render(c, c["cams"][k:k + 1]) for k in range(len(c["cams"]))])
    assert torch.equal(batch.view(torch.int32), single.view(torch.int32))
    c = C.by_name("64x48_F600_K3")
    batch = _render(c)
    single = torch.cat([_render(c, c["cams"][k:k + 1]) for k in range(3)])
    assert torch.equal(batch.view(torch.int32), single.view(torch.int32))


def test_binning_statistics_and_the_oversize_list():
    from gs_train import mesh_depth as M
    c = C.by_name("oversize_frame_filling")
    st = {}
    M.render_mesh_distance(c["vertices"], c["faces"], c["cams"][:, :4], c["cams"][:, 4:7], c["cams"][:, 7:], 64, 48, stats=st)
    assert st["oversize"] == 1 and st["references"] > 1 and st["longest_run"] >= 2
    c = C.by_name("fan_5000_in_one_tile")
    st = {}
    M.render_mesh_distance(c["vertices"], c["faces"], c["cams"][:, :4], c["cams"][:, 4:7], c["cams"][:, 7:], 32, 32, stats=st)
    assert st.pop("bin_us") > 0 and st.pop("cast_us") > 0
    assert st == {"references": 5000, "oversize": 0, "longest_run": 5000, "occupied_tiles": 1}


def test_tensor_inputs_and_modes_agree():
    """Device tensors in place of arrays give the same bits; camera z is the distance over |d|."""
    from gs_train import mesh_depth as M
    c = C.by_name("64x48_F600_K3")
    dev = torch.device("cuda")
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    cams = c["cams"]
    a = M.render_mesh_distance(t(c["vertices"], torch.float32), t(c["faces"], torch.int32), t(cams[:, :4], torch.float64),
                               t(cams[:, 4:7], torch.float64), t(cams[:, 7:], torch.float64), 64, 48)
    assert torch.equal(a, _render(c))
    z = _render(c, depth="z").cpu().numpy()
    for k in range(3):
        dx, dy = R.rays(cams[k], 64, 48)
        ln = np.sqrt(dx * dx + dy * dy + 1).reshape(48, 64)
        hit = z[k] > 0
        assert np.array_equal(hit, a[k].cpu().numpy() > 0)
        assert np.abs(z[k] * ln - a[k].cpu().numpy())[hit].max() <= 4 * 2.0 ** -24 * a[k].max().item()


@pytest.mark.parametrize("case", C.encode_cases(), ids=lambda e: e[0])
def test_encode_equals_float64_exactly(case):
    from gs_train import mesh_depth as M
    name, dist, kw = case
    maps = M.encode_depth_maps(torch.tensor(dist, device="cuda"), **kw)
    u16, scale, offset = R.encode64(dist, **kw)
    assert maps.u16.shape == dist.shape and maps.scale.dtype == np.float64
    assert np.array_equal(maps.u16.cpu().numpy(), u16.astype(np.int32)), name
    assert np.array_equal(maps.scale, scale) and np.array_equal(maps.offset, offset), name
    again = M.encode_depth_maps(torch.tensor(dist, device="cuda"), **kw)
    assert torch.equal(again.u16, maps.u16) and np.array_equal(again.scale, maps.scale)


def test_end_to_end_invdepth_of_a_rendered_frame(tmp_path):
    """Render 64 x 48, encode, write the PNGs and depth_params.json, read them back: invdepth() equals the
    float64 pipeline on the float64 ray cast wherever the quantiser's input is not within the distance
    bar of a code step (there the 4 mm step may fall either way)."""
    from gs_train import mesh_depth as M
    c = C.by_name("64x48_F600_K3")
    dist = _render(c)
    maps = M.encode_depth_maps(dist)
    host = dist.cpu().numpy()
    u16, scale, offset = R.encode64(host)  # the encode of the kernel's own distances: exact
    assert np.array_equal(maps.u16.cpu().numpy(), u16.astype(np.int32)) and np.array_equal(maps.scale, scale)
    names = [f"cam{k}/{k:05d}_X_f1.jpg" for k in range(3)]
    maps.save(tmp_path / "depths", names)
    M.write_depth_params(tmp_path / "depth_params.json", names + ["cam9/none.jpg"], (names, maps))
    params = M.read_depth_params(tmp_path / "depth_params.json")
    assert params["cam9/none"]["scale"] == 0.0 and len(params) == 4
    inv, mask = maps.invdepth(), maps.depth_mask()
    for k, r in enumerate(C.reference(c["name"])):
        png = M.load_png16(tmp_path / "depths" / f"cam{k}" / f"{k:05d}_X_f1.png")
        assert np.array_equal(png, u16[k])
        p = params[f"cam{k}/{k:05d}_X_f1"]
        assert (p["scale"], p["offset"]) == (scale[k], offset[k]) and p["scale"] > 0
        want = np.maximum((png.astype(np.float32) / np.float32(65536.0)) * np.float32(p["scale"]) + np.float32(p["offset"]), 0)
        assert np.array_equal(inv[k][0].cpu().numpy(), want)
        assert np.array_equal(mask[k][0].cpu().numpy() > 0, want > 0)
        # against the float64 ray cast: the same depth code where no step is within the bar
        d64 = r["distance"]
        safe = ~r["boundary"] & (d64 > 0) & (R.code_steps(d64) > bar_units() * r["scale"] + 2.0 ** -24 * d64)
        assert safe.mean() > 0.5
        dep_gpu, _ = R.depth_of(host[k], True)
        dep_64, _ = R.depth_of_mm(1000.0 * d64)
        assert np.array_equal(dep_gpu[safe], dep_64[safe])


def test_errors_and_no_ops():
    from gs_train import mesh_depth as M
    c = C.by_name("16x16_F2_K3")
    q, t, k = c["cams"][:, :4], c["cams"][:, 4:7], c["cams"][:, 7:]
    assert M.render_mesh_distance(c["vertices"], c["faces"], q[:0], t[:0], k[:0], 16, 16).shape == (0, 16, 16)
    assert M.render_mesh_distance(c["vertices"], c["faces"], q, t, k, 0, 16).shape == (3, 16, 0)
    assert M.render_mesh_distance(c["vertices"], c["faces"], q, t, k, 16, 0).shape == (3, 0, 16)
    none = M.render_mesh_distance(c["vertices"], c["faces"][:0], q, t, k, 16, 16)
    assert none.shape == (3, 16, 16) and not none.any()
    # a camera that is not finite, or without a focal length, sees nothing; the others are untouched
    cams = c["cams"].copy()
    cams[0, 5] = np.nan
    cams[2, 7] = 0.0
    out = M.render_mesh_distance(c["vertices"], c["faces"], cams[:, :4], cams[:, 4:7], cams[:, 7:], 16, 16)
    assert not out[0].any() and not out[2].any() and torch.equal(out[1], _render(c)[1])
    # the C entry points themselves
    L = M.lib()
    v = torch.tensor(c["vertices"], device="cuda")
    f = torch.tensor(c["faces"], device="cuda")
    cd = torch.tensor(c["cams"], device="cuda")
    o = torch.full((3, 16, 16), 7.0, device="cuda")
    s = torch.empty(L.gsr_mesh_distance_scratch_bytes(3, 2), dtype=torch.uint8, device="cuda")
    p = lambda x: x.data_ptr()
    assert L.gsr_mesh_distance_maps(4, p(v), 0, p(f), 3, p(cd), 16, 16, 0.0, 10.0, 0, p(s), p(o), None, None) == 0
    torch.cuda.synchronize()
    assert not o.any()  # F = 0 with a frame: zeroed
    assert L.gsr_mesh_distance_maps(4, p(v), 2, p(f), 3, p(cd), 16, 16, 0.0, 10.0, 0, None, p(o), None, None) != 0
    assert b"gsr_mesh_distance_maps" in L.gsr_last_error()
    with pytest.raises(ValueError):
        M.encode_depth_maps(torch.zeros((2, 3), device="cuda"))
    with pytest.raises(ValueError):
        M.encode_depth_maps(torch.zeros((1, 2, 3), device="cuda"), min_depth=-1.0)
    with pytest.raises(ValueError):
        M.encode_depth_maps(torch.zeros((1, 2, 3), device="cuda"), max_depth=0.0)
    e = M.encode_depth_maps(torch.zeros((0, 4, 4), device="cuda"))
    assert e.u16.shape == (0, 4, 4) and e.scale.shape == (0,) and e.invdepth() == []
