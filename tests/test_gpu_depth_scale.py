"""GPU tests of the depth scale fit (gs_train/depth_scale.py, csrc/depth_scale.hip) against the numpy
restatement of its rule (tests/depth_scale_ref.py), on every case of tests/depth_scale_cases.py and on
the reference-generated tests/golden/depth_scale.npz.

What the kernel selects is exact and its inputs are bit-defined: n_valid, the fitted flag, t_colmap and
t_mono must equal the restatement's.  The two mean absolute deviations are fp64 sums of n non-negative
terms in the kernel's own fixed order: within (n + 8) 2^-52 relative of the exactly rounded ones; scale
and offset within the bounds that follow."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import depth_scale_cases as C
import depth_scale_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "depth_scale.npz")
FIELDS = ("scale", "offset", "n_valid", "t_colmap", "s_colmap", "t_mono", "s_mono", "fitted", "nan_seen")
_FITS = {}


def _fit(sc, missing="origin", **kw):
    from gs_train.depth_scale import fit_depth_scales
    q, t, sizes, ptr, xy, pid, maps, index = C.arrays(sc)
    a = dict(qvecs=q, tvecs=t, sizes=sizes, obs_ptr=ptr, obs_xy=xy, obs_point_id=pid, point_id=sc["point_id"],
             point_xyz=sc["point_xyz"], maps=maps, map_index=index, missing=missing, device=DEV)
    a.update(kw)
    return fit_depth_scales(**a)


def _case_fit(name, missing):
    if (name, missing) not in _FITS:
        _FITS[name, missing] = _fit(C.by_name(name), missing)
    return _FITS[name, missing]


def _close(got, want, tol, what):
    if np.isnan(want):
        assert np.isnan(got), what
    elif np.isinf(want):
        assert got == want, what
    else:
        assert abs(got - want) <= tol, (what, got, want, tol)


def check(fit, k, want, what):
    if want is None:
        assert k in fit.no_map and not fit.fitted[k] and fit.scale[k] == 0 and fit.offset[k] == 0, what
        return
    assert k not in fit.no_map, what
    assert int(fit.n_valid[k]) == want["n_valid"], what
    assert bool(fit.fitted[k]) == want["fitted"] and bool(fit.nan_seen[k]) == want["nan_seen"], what
    assert fit.t_colmap[k] == want["t_colmap"] and fit.t_mono[k] == want["t_mono"], what
    e = (want["n_valid"] + 8) * 2.0 ** -52
    _close(fit.s_colmap[k], want["s_colmap"], e * want["s_colmap"], what + " s_colmap")
    _close(fit.s_mono[k], want["s_mono"], e * want["s_mono"], what + " s_mono")
    _close(fit.scale[k], want["scale"], 2 * e * abs(want["scale"]), what + " scale")
    _close(fit.offset[k], want["offset"], e * (abs(want["t_colmap"]) + abs(want["t_mono"] * want["scale"])),
           what + " offset")


SCENES = [sc["name"] for sc in C.scenes()]


@pytest.mark.parametrize("missing", C.MODES)
@pytest.mark.parametrize("name", SCENES)
def test_cases_equal_the_restatement(name, missing):
    fit = _case_fit(name, missing)
    sc = C.by_name(name)
    assert len(fit.scale) == len(sc["images"])
    for k, (im, want) in enumerate(zip(sc["images"], C.reference(name, missing))):
        check(fit, k, want, f"{name}/{im['name']}[{missing}]")


def test_fixture_equals_the_restatement():
    """The reference-generated images, grouped by map size (one size per call)."""
    g = np.load(GOLD)
    ims = []
    for k in range(int(g["n"])):
        ims.append(dict(name=f"im{k}", q=g[f"q_{k}"], t=g[f"t_{k}"], width=int(g[f"wh_{k}"][0]), height=int(g[f"wh_{k}"][1]),
                        xy=g[f"xy_{k}"], pid=g[f"pid_{k}"], u16=g[f"u16_{k}"] if int(g[f"has_map_{k}"]) else None))
    sizes = sorted({im["u16"].shape for im in ims if im["u16"] is not None})
    assert len(ims) >= 8 and len(sizes) >= 3
    seen = 0
    for j, (Hd, Wd) in enumerate(sizes):
        group = [im for im in ims if im["u16"] is not None and im["u16"].shape == (Hd, Wd)]
        if j == 0:
            group += [im for im in ims if im["u16"] is None]
        sc = dict(name="fixture", Hd=Hd, Wd=Wd, point_id=g["point_id"], point_xyz=g["point_xyz"], images=group)
        fit = _fit(sc)
        for k, im in enumerate(group):
            want = R.fit_image(im["q"], im["t"], im["width"], im["height"], im["xy"], im["pid"], g["point_id"],
                               g["point_xyz"], im["u16"])
            check(fit, k, want, im["name"])
            seen += 1
    assert seen == len(ims)


def _bits(fit):
    return [np.ascontiguousarray(getattr(fit, f)).view(np.uint8).tobytes() for f in FIELDS]


def test_two_runs_are_bit_equal():
    for name in ("counts", "depths_ids_maps"):
        assert _bits(_fit(C.by_name(name))) == _bits(_case_fit(name, "origin"))


def test_obs_index_equals_the_materialised_arrays():
    """A permuted and partial obs_index (every camera keeps a shuffled two thirds of its observations),
    host or device, against the arrays gathered on the host; and Chunk's form: point rows of a subset."""
    sc = C.by_name("counts")
    q, t, sizes, ptr, xy, pid, maps, index = C.arrays(sc)
    rng = np.random.default_rng(7)
    parts = []
    for m in range(len(q)):
        o = rng.permutation(np.arange(ptr[m], ptr[m + 1]))
        parts.append(o[:len(o) - len(o) // 3])
    obs_index = np.concatenate(parts).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    direct = _fit(sc, obs_ptr=offsets, obs_xy=xy[obs_index], obs_point_id=pid[obs_index])
    via = _fit(sc, obs_ptr=None, obs_index=torch.from_numpy(obs_index).to(DEV), obs_offsets=offsets)
    assert _bits(via) == _bits(direct)
    assert _bits(_fit(sc, obs_index=obs_index, obs_offsets=offsets)) == _bits(direct)
    assert not np.array_equal(direct.n_valid, _case_fit("counts", "origin").n_valid)  # it is a different problem
    for k, m in enumerate(range(len(q))):  # and the restatement's answer on it
        im = sc["images"][m]
        want = R.fit_image(im["q"], im["t"], im["width"], im["height"], xy[parts[m]], pid[parts[m]], sc["point_id"],
                           sc["point_xyz"], im["u16"])
        check(via, k, want, im["name"])


@pytest.mark.parametrize("missing", C.MODES)
def test_a_chunks_call(missing):
    """The per-chunk form: some of the cameras, their kept observations through obs_index / obs_offsets
    into the scene's arrays, and a point table of the chunk's rows only -- ids of the other points are now
    ids without a row, or ids at and above T.  The cameras are moved back by 1 so that an origin point
    (missing="origin") sits at z = 1, in front of them."""
    sc = C.by_name("counts")
    q, t, sizes, ptr, xy, pid, maps, index = C.arrays(sc)
    rng = np.random.default_rng(11)
    rows = np.sort(rng.permutation(len(sc["point_id"]))[:30])
    cams = np.array([3, 4, 9, 13, 16], np.int64)
    parts = [np.sort(rng.permutation(np.arange(ptr[m], ptr[m + 1]))[:(ptr[m + 1] - ptr[m]) * 3 // 4]) for m in cams]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    back = np.array([0.0, 0.0, 1.0])
    fit = _fit(sc, missing, tvecs=t + back, obs_ptr=None, point_id=sc["point_id"][rows],
               point_xyz=torch.from_numpy(sc["point_xyz"][rows]).to(DEV), maps=maps[index[cams]], map_index=None,
               cameras=cams, obs_index=torch.from_numpy(np.concatenate(parts)).to(DEV), obs_offsets=offsets)
    modes = set()
    for k, m in enumerate(cams):
        im = sc["images"][m]
        want = R.fit_image(im["q"], im["t"] + back, im["width"], im["height"], xy[parts[k]], pid[parts[k]],
                           sc["point_id"][rows], sc["point_xyz"][rows], im["u16"], missing)
        check(fit, k, want, im["name"])
        modes.add(want["fitted"] and np.isfinite(want["scale"]))
    assert modes == {False, True}


def test_camera_subset_and_map_forms():
    sc = C.by_name("depths_ids_maps")
    whole = _case_fit(sc["name"], "origin")
    q, t, sizes, ptr, xy, pid, maps, index = C.arrays(sc)
    cams = np.array([13, 0, 14, 5, 5, 8], np.int64)  # out of order, one twice, one without a map
    sub = _fit(sc, cameras=cams, map_index=index[cams])
    assert sub.no_map == [2] and np.array_equal(sub.cameras, cams)
    for f in FIELDS:
        assert np.array_equal(getattr(sub, f), getattr(whole, f)[cams], equal_nan=True), f
    # the maps as DepthMaps.u16 holds them (int32 on the device) and as the uint16 bits
    as_i32 = torch.from_numpy(maps.astype(np.int32)).to(DEV)
    as_bits = torch.from_numpy(maps.view(np.int16)).to(DEV)
    assert _bits(_fit(sc, maps=as_i32)) == _bits(whole) and _bits(_fit(sc, maps=as_bits)) == _bits(whole)
    # params: the cameras without a map are left out, the others carry scale and offset
    names = [f"cam0/{im['name']}.jpg" for im in sc["images"]]
    p = whole.params(names)
    assert len(p) == len(names) - 1 and "cam0/absent_map" not in p
    assert p["cam0/behind_camera"] == (float(whole.scale[0]), float(whole.offset[0]))


def test_depth_maps_go_into_the_view_store():
    from gs_train.views import ViewStore
    sc = C.by_name("positions_s1")
    fit = _case_fit(sc["name"], "origin")
    dm = fit.depth_maps()
    n = len(sc["images"])
    assert dm.u16.shape == (n, sc["Hd"], sc["Wd"]) and dm.u16.dtype == torch.int32
    assert np.array_equal(dm.scale, fit.scale) and np.array_equal(dm.offset, fit.offset) and fit.fitted.all()
    inv = dm.invdepth()
    store = ViewStore(DEV, slots=2)
    for _ in range(n):
        store.add(image=np.zeros((sc["Hd"], sc["Wd"], 3), np.uint8))
    store.add_depth_maps(dm)
    for k in (0, n - 1):
        assert (fit.scale[k] > 0) and inv[k] is not None
        assert torch.equal(store.mono_invdepths[k], inv[k])
    # a camera without a map, a flat map (inf / -inf) and an unfitted one give views without depth
    d = _case_fit("depths_ids_maps", "origin")
    dm = d.depth_maps()
    names = [im["name"] for im in C.by_name("depths_ids_maps")["images"]]
    for nm in ("absent_map", "flat_map", "range_below_1e-3", "range_above_1e-3"):
        k = names.index(nm)
        assert dm.scale[k] == 0 and dm.offset[k] == 0 and dm.invdepth()[k] is None
    assert not dm.u16[names.index("absent_map")].any()
