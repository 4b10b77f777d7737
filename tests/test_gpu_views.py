"""GPU tests of the training-view stage (csrc/views.hip, gs_train/views.py): the Lanczos resize kernel
against the integer restatement and the reference's PILtoTorch fixture, the plan's upload counter, the
expansion against the float32 restatement bit for bit and against torch's CPU arithmetic, the refusals,
the plane sets' reuse, a NativeTrainStep fed by the store against one fed by lists, and the evaluator."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

import views_cases as C
import views_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "views.npz")
LANCZOS = C.lanczos_cases()
EXPAND = C.expand_cases()
KEYS = ("image", "mask", "u16", "scale", "offset", "size", "depth_only", "test_half", "depth_valid")
PLANES = (("gts", "original_image"), ("alpha_masks", "alpha_mask"), ("mono_invdepths", "invdepthmap"),
          ("depth_masks", "depth_mask"))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("c", LANCZOS, ids=[c["name"] for c in LANCZOS])
def test_resize_equals_the_restatement(c):
    from gs_train.views import ResizePlan, resize_lanczos
    want = R.resize_lanczos_ref(c["image"], c["size"])
    H, W = c["image"].shape[:2]
    plan = ResizePlan(W, H, *c["size"])
    got = resize_lanczos(c["image"], c["size"], device=DEV, plan=plan)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    diff = int((got.cpu().numpy() != want).sum())
    print(f"{c['name']}: {diff} of {want.size} samples differ")
    assert diff == 0
    # the tables went up once; the second resize of the geometry uploads nothing and gives the same image
    assert plan.uploads == 1
    again = resize_lanczos(torch.from_numpy(c["image"]).to(DEV), c["size"], plan=plan)
    assert plan.uploads == 1 and torch.equal(again, got)


def test_resize_equals_the_reference_fixture():
    from gs_train.views import resize_lanczos
    g = np.load(GOLD)
    for k in range(int(g["n"])):
        img, size, out = g[f"in_{k}"], tuple(int(v) for v in g[f"size_{k}"]), g[f"out_{k}"]
        got = resize_lanczos(img, size, device=DEV)
        got = got[None] if got.dim() == 2 else got.permute(2, 0, 1)
        assert np.array_equal(bits((got.cpu() / 255.0).numpy()), bits(out)), k  # PILtoTorch's own tensor


def _store_of(c, slots=2):
    from gs_train.views import ViewStore
    store = ViewStore(DEV, slots=slots)
    k = store.add(image=c["image"], mask=c["mask"], invdepth_u16=c["u16"], scale=c["scale"], offset=c["offset"],
                  resolution=c["size"], depth_only=c["depth_only"], test_half=c["test_half"],
                  depth_valid=c["depth_valid"])
    return store, k


@pytest.mark.parametrize("c", EXPAND, ids=[c["name"] for c in EXPAND])
def test_expand_equals_the_restatement_bit_for_bit(c):
    want = R.expand_ref(**{k: c[k] for k in KEYS})
    store, k = _store_of(c)
    w, h = c["size"]
    for seq, name in PLANES:
        got = getattr(store, seq)[k]
        if want[name] is None:
            assert got is None, name
            continue
        assert got.dtype == torch.float32 and got.is_contiguous() and got.data_ptr() % 16 == 0, name
        assert tuple(got.shape) == want[name].shape == ((3 if name == "original_image" else 1), h, w)
        diff = int((bits(got.cpu().numpy()) != bits(want[name])).sum())
        print(f"{c['name']} {name}: {diff} of {want[name].size} values differ in their bits")
        assert diff == 0, name
    assert store.expansions == 1  # one launch made all the planes
    v = store.view(k)
    assert (v.image_width, v.image_height, v.is_depth_only) == (w, h, c["depth_only"])
    assert v.depth_reliable == (want["invdepthmap"] is not None) and v.original_image is store.gts[k]
    if c["u16"] is None:  # no depth involved: torch's own CPU arithmetic of PILtoTorch and Camera.__init__
        alpha = torch.ones(1, h, w) if c["mask"] is None else (torch.from_numpy(c["mask"]) / 255.0)[None]
        if c["test_half"] == "left":
            alpha[..., :w // 2] = 0
        elif c["test_half"] == "right":
            alpha[..., w // 2:] = 0
        img = (torch.from_numpy(c["image"]) / 255.0).permute(2, 0, 1).clamp(0.0, 1.0) * alpha
        assert torch.equal(store.gts[k].cpu(), img) and torch.equal(store.alpha_masks[k].cpu(), alpha)


def test_store_resizes_image_and_mask_to_the_resolution():
    from gs_train.views import ViewStore, target_resolution
    rng = np.random.default_rng(8)
    img, mask = C.lanczos_image(60, 84, 3, 1), rng.integers(0, 256, (60, 84), dtype=np.uint8)
    res = target_resolution(84, 60, resolution=2)
    assert res == (42, 30)
    store = ViewStore(DEV)
    k = store.add(image=torch.from_numpy(img), mask=mask, resolution=res)
    want = R.expand_ref(image=R.resize_lanczos_ref(img, res), mask=R.resize_lanczos_ref(mask, res))
    assert np.array_equal(bits(store.gts[k].cpu().numpy()), bits(want["original_image"]))
    assert np.array_equal(bits(store.alpha_masks[k].cpu().numpy()), bits(want["alpha_mask"]))
    assert store.mono_invdepths[k] is None and store.depth_masks[k] is None
    nb = store.nbytes()
    assert nb["compact"] == 42 * 30 * 4 and nb["expanded"] == 42 * 30 * 16 and nb["planes"] == 2 * 42 * 30 * 16


def test_refusals_on_the_device():
    from gs_train.views import ViewStore, resize_lanczos
    with pytest.raises(ValueError, match="premultiplies"):
        resize_lanczos(torch.zeros(8, 8, 4, dtype=torch.uint8, device=DEV), (4, 4))
    store = ViewStore(DEV)
    with pytest.raises(ValueError, match="premultiplies"):
        store.add(image=torch.zeros(8, 8, 4, dtype=torch.uint8, device=DEV))
    for bad in (torch.zeros(8, 8, 3, dtype=torch.uint8, device=DEV), torch.zeros(8, 8, device=DEV),
                np.zeros((8, 8), np.uint16)):
        with pytest.raises(ValueError, match="single-channel"):
            store.add(image=np.zeros((8, 8, 3), np.uint8), mask=bad)
    assert len(store) == 0


def test_plane_sets_are_reused_least_recently_used_first():
    from gs_train.views import ViewStore
    store = ViewStore(DEV, slots=2)
    cases = [EXPAND[1], EXPAND[2], EXPAND[0]]  # 12 x 20 each: with a mask, with depth, plain
    for c in cases:
        store.add(image=c["image"], mask=c["mask"], invdepth_u16=c["u16"], scale=c["scale"], offset=c["offset"])
    want = [R.expand_ref(**{k: c[k] for k in KEYS}) for c in cases]
    g0, a0 = store.gts[0], store.alpha_masks[0]
    g1, d1 = store.gts[1], store.mono_invdepths[1]
    assert store.expansions == 2
    assert store.gts[0] is g0 and store.alpha_masks[0] is a0 and store.expansions == 2  # no launch
    assert np.array_equal(bits(g1.cpu().numpy()), bits(want[1]["original_image"]))  # view 1 is still whole
    assert np.array_equal(bits(d1.cpu().numpy()), bits(want[1]["invdepthmap"]))
    g2 = store.gts[2]  # takes view 1's set: view 0 was touched after it
    assert store.expansions == 3 and g2.data_ptr() == g1.data_ptr()
    assert np.array_equal(bits(g1.cpu().numpy()), bits(want[2]["original_image"]))  # overwritten by view 2
    assert np.array_equal(bits(g0.cpu().numpy()), bits(want[0]["original_image"]))  # view 0 untouched
    assert store.gts[0] is g0 and store.expansions == 3
    assert store.gts[1] is not g1 and store.expansions == 4  # view 1 again: into view 2's set
    assert len(store.gts) == len(store.depth_masks) == 3 and [t is None for t in store.mono_invdepths] == [True, False, True]


def test_add_depth_maps_attaches_a_batch():
    from gs_train.mesh_depth import DepthMaps
    from gs_train.views import ViewStore
    cases = [EXPAND[0], EXPAND[1]]
    store = ViewStore(DEV, slots=2)
    for c in cases:
        store.add(image=c["image"], mask=c["mask"])
    assert store.mono_invdepths[1] is None
    rng = np.random.default_rng(5)
    u16 = rng.integers(0, 65536, (2, 24, 40)).astype(np.int32)
    maps = DepthMaps(torch.from_numpy(u16).to(DEV), np.array([0.0, 0.75]), np.array([0.1, -0.2]))
    store.add_depth_maps(maps, k0=0)
    assert store.mono_invdepths[0] is None  # scale 0: no depth for the view
    want = R.expand_ref(image=cases[1]["image"], mask=cases[1]["mask"], u16=u16[1], scale=0.75, offset=-0.2)
    assert np.array_equal(bits(store.mono_invdepths[1].cpu().numpy()), bits(want["invdepthmap"]))
    assert np.array_equal(bits(store.depth_masks[1].cpu().numpy()), bits(want["depth_mask"]))
    with pytest.raises(ValueError):
        store.add_depth_maps(maps, k0=1)


# ---- a step fed by the store ----------------------------------------------------------------------

def _compact_problem():
    """harness.make_problem's scene at 96 x 64, its targets quantised as files hold them: RGB8, mask8,
    and the inverse depth as 16 bits with a scale and an offset; the last view is depth-only."""
    from gs_train.harness import make_problem
    from gs_train.native_step import NativeTrainStep
    from gs_train.synthetic import orbit_cameras
    W, H, n = 96, 64, 3
    torch.manual_seed(0)
    ts = make_problem(3000, W, H, n_views=n, seed=1, step_cls=NativeTrainStep, alpha=True, depth_only=1)
    views = []
    for k in range(n):
        d = ts.mono[k][0].cpu()
        scale = float(d.max()) * 1.01 + 1e-3
        v = dict(u16=torch.clamp(torch.round((d + 0.01) / scale * 65536.0), 0, 65535).to(torch.int32).numpy(),
                 scale=scale, offset=-0.01, image=None, mask=None)
        if not ts.depth_only[k]:
            v["image"] = torch.round(ts.gts[k].clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()
            v["mask"] = (ts.amask[k][0] * 255).to(torch.uint8).cpu().numpy()
        views.append(v)
    return ts.g, orbit_cameras(n, W, H, fovx_deg=60.0), views, ts.depth_only, (W, H)


def _lists_with_torch(views, dev):
    """The planes as PILtoTorch and Camera.__init__ make them, with torch on the CPU."""
    gts, alphas, monos, dmasks = [], [], [], []
    for v in views:
        h, w = v["u16"].shape
        alpha = torch.ones(1, h, w) if v["mask"] is None else (torch.from_numpy(v["mask"]) / 255.0)[None]
        if v["image"] is None:
            gts.append(None)
        else:
            gts.append(((torch.from_numpy(v["image"]) / 255.0).permute(2, 0, 1).clamp(0.0, 1.0) * alpha).contiguous())
        m = torch.from_numpy(v["u16"].astype(np.float32)) / float(2 ** 16)
        m = m * v["scale"] + v["offset"]
        m[m < 0] = 0
        monos.append(m[None])
        alphas.append(alpha)
        dmasks.append(alpha.clone())
    put = lambda ts: [None if t is None else t.to(dev) for t in ts]
    return put(gts), put(alphas), put(monos), put(dmasks)


def test_native_step_fed_by_the_store_equals_one_fed_by_lists():
    from helpers import deterministic
    from gs_train.native_step import NativeTrainStep
    from gs_train.views import ViewStore
    names = ("_xyz", "_features", "_opacity", "_scaling", "_rotation", "_exposure")
    out = {}
    with deterministic():
        for fed in ("lists", "store"):
            g, cams, views, depth_only, (W, H) = _compact_problem()
            if fed == "lists":
                gts, alphas, monos, dmasks = _lists_with_torch(views, DEV)
                alphas = [None if d else a for a, d in zip(alphas, depth_only)]
            else:
                store = ViewStore(DEV, slots=2)
                for v in views:
                    store.add(image=v["image"], mask=v["mask"], invdepth_u16=v["u16"], scale=v["scale"], offset=v["offset"])
                assert store.depth_only == depth_only
                gts, alphas, monos, dmasks = store.gts, store.alpha_masks, store.mono_invdepths, store.depth_masks
            ts = NativeTrainStep(g, cams, gts, W, H, mono_invdepths=monos, depth_masks=dmasks, alpha_masks=alphas,
                                 depth_only=depth_only, iterations=30)
            torch.manual_seed(3)  # the random backgrounds
            losses = torch.stack([ts.step().clone() for _ in range(6)])  # views 0, 1, 2 (depth-only), twice
            out[fed] = (losses, [getattr(ts.g, n).detach().clone() for n in names])
            assert not ts._copies  # every plane was 16-byte aligned: _aligned never copied
    (la, pa), (lb, pb) = out["lists"], out["store"]
    print("losses by lists", la.tolist(), "by the store", lb.tolist())
    assert bool(torch.isfinite(la).all()) and float(la.min()) > 0
    assert torch.equal(la, lb)
    for n, x, y in zip(names, pa, pb):
        assert torch.equal(x, y), n


def test_evaluator_accepts_a_store_view():
    from gs_train.evaluate import Evaluator
    from gs_train.views import ViewStore
    c = EXPAND[3]  # 48 x 64 with a mask and a depth map
    store, k = _store_of(c)
    w, h = c["size"]
    g = torch.Generator().manual_seed(2)
    pkg = {"render": torch.rand((3, h, w), generator=g).to(DEV), "depth": (torch.rand((1, h, w), generator=g) * 0.5).to(DEV)}
    want = R.expand_ref(**{key: c[key] for key in KEYS})
    as_dict = {name: torch.from_numpy(want[name]).to(DEV) for name in ("original_image", "alpha_mask", "invdepthmap")}
    a = Evaluator().add_view(pkg, store.view(k))
    b = Evaluator().add_view(pkg, as_dict)
    assert torch.equal(a, b) and float(a[0, 4]) > 0
