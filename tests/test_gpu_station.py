"""GPU tests of the station render (csrc/station.hip, gs_train/station.py) on the inputs of
tests/station_cases.py.

The yardstick is the fused single-view cut frame of the same face at the same campos
(_C.rasterize_gaussians(..., render_indices, parent_indices, weights, ..., need_backward=False)),
itself held to the oracle by test_gpu_lod.py.  For every face: K equal, the (F, R) radii equal,
colour and inverse depth bitwise equal -- station_rows forms the blend, the covariance and the colour
with the device functions the fused frame uses, and the library is compiled without FMA contraction.
The largest deviation (0 when bitwise equal) goes to $GSR_PARITY_RECORD
(profiles/r26_station_margins.jsonl)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import station_cases as SC
from helpers import record_margins

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _renderer(h):
    from gs_train.station import StationRenderer
    return StationRenderer(h, DEV)


def _check(name, h, cams, ri, pi, w, sr=None, D=3, bg=SC.BG, center=None):
    """One station call against the single-view frame of every face.  Returns (images, invdepths,
    radii, renderer)."""
    sr = sr or _renderer(h)
    ctr = cams[0]["campos"] if center is None else center
    img, inv, radii = sr.render_cut(cams, ri, pi, w, center=ctr, bg=bg, sh_degree=D)
    torch.cuda.synchronize()
    R = int(ri.shape[0])
    assert tuple(img.shape) == (len(cams), 3, cams[0]["H"], cams[0]["W"]) and tuple(radii.shape) == (len(cams), R)
    worst = 0.0
    for f, cam in enumerate(cams):
        yc = dict(cam, campos=ctr)
        K, col, dep, rad = SC.single_view(h, yc, ri, pi, w, DEV, bg=bg, sh_degree=D)
        rows = sr.face_rows(f)
        src = rows["src"].long()
        assert sr.last_K[f] == K, (name, f, sr.last_K[f], K)
        assert torch.equal(radii[f], rad), (name, f, int((radii[f] != rad).sum()))
        # the kept rows: in cut order, no row twice, every drawn row among them
        assert src.numel() == sr.last_kept[f]
        assert bool((src[1:] > src[:-1]).all()) and (src.numel() == 0 or (0 <= int(src[0]) and int(src[-1]) < R))
        drawn = rad > 0
        keep = torch.zeros(R, dtype=torch.bool, device=DEV)
        keep[src] = True
        assert bool(keep[drawn].all()), (name, f, "a row with radii > 0 was dropped")
        worst = max(worst, float((img[f] - col).abs().max()), float((inv[f] - dep).abs().max()))
        assert torch.equal(img[f], col), (name, f, "colour", float((img[f] - col).abs().max()))
        assert torch.equal(inv[f], dep), (name, f, "inverse depth", float((inv[f] - dep).abs().max()))
    record_margins("station_" + name, max_abs_dev=worst, faces=len(cams), rows=R)
    return img, inv, radii, sr


def test_one_face_equals_the_single_view_frame():
    h = SC.shell(DEV)
    ri, pi, w = SC.cut(DEV)
    assert 1000 < ri.shape[0] < h["means3D"].shape[0]
    _, _, radii, sr = _check("f1", h, SC.faces(4)[:1], ri, pi, w)
    assert 0 < sr.last_kept[0] < ri.shape[0] and int((radii[0] > 0).sum()) > 100


def test_four_horizontal_faces_drop_rows_above_and_below():
    h = SC.shell(DEV)
    ri, pi, w = SC.cut(DEV)
    cams = SC.faces(4)
    _, _, radii, sr = _check("f4", h, cams, ri, pi, w)
    R = ri.shape[0]
    hits = torch.zeros(R, dtype=torch.int32, device=DEV)
    for f in range(4):
        hits[sr.face_rows(f)["src"].long()] += 1
    unseen = (radii > 0).sum(0) == 0
    assert int(unseen.sum()) > 0, "the shell has rows above and below the four faces"
    # such rows reach no face's compact rows unless a face's own cull keeps them (none does: the keep
    # test is the preprocess's cull, so kept == drawn)
    assert int(hits[unseen].sum()) == 0
    assert int((hits >= 2).sum()) > 0, "rows on a cube edge are kept by two faces"
    assert sum(sr.last_kept) < 2 * R  # a quarter of the sphere each, not the half space


def test_six_faces_through_render():
    """render(): the cut and the weights made once inside, skybox rows appended."""
    h = SC.shell(DEV, skybox=3000)
    cams = SC.faces(6)
    sr = _renderer(h)
    img, inv, radii = sr.render(cams, SC.TAU, bg=SC.BG)
    ri, pi, w = SC.cut(DEV, skybox=3000)
    for a, b in zip(sr.last_cut, (ri, pi, w)):
        assert torch.equal(a, b)
    img2, inv2, radii2, _ = _check("f6_sky3000", h, cams, ri, pi, w, sr=sr)
    assert torch.equal(img, img2) and torch.equal(inv, inv2) and torch.equal(radii, radii2)
    S, R = 3000, ri.shape[0]
    assert int((radii[:, R - S:] > 0).sum()) > 0, "skybox rows are drawn"
    seen = (radii > 0).sum(0)
    assert int((seen == 0).sum()) < R // 4  # six faces cover the sphere (rows too faint or small aside)


def test_no_skybox():
    h = SC.shell(DEV, skybox=0)
    ri, pi, w = SC.cut(DEV, skybox=0)
    _check("f6_sky0", h, SC.faces(6), ri, pi, w)


def test_face_towards_an_empty_half_space_is_background():
    """The cut without the rows of the z > 0 hemisphere (child and parent both behind face 0, so
    the blend is too): face 0 keeps nothing and is the background."""
    h = SC.shell(DEV)
    ri, pi, w = SC.cut(DEV)
    z = h["means3D"][:, 2]
    back = (z[ri.long()] < 0) & (z[pi.long()] < 0)
    ri2, pi2, w2 = ri[back].contiguous(), pi[back].contiguous(), w[back].contiguous()
    assert ri2.shape[0] > 1000
    cams = SC.faces(4)
    img, inv, radii, sr = _check("empty_face", h, cams, ri2, pi2, w2)
    assert sr.last_kept[0] == 0 and sr.last_K[0] == 0 and sr.last_kept[2] > 0
    assert int(radii[0].abs().sum()) == 0
    bg = torch.tensor(SC.BG, device=DEV).view(3, 1, 1).expand(3, SC.FACE, SC.FACE)
    assert torch.equal(img[0], bg) and int((inv[0] != 0).sum()) == 0


def test_empty_cut_is_background():
    h = SC.shell(DEV)
    e32 = torch.empty(0, dtype=torch.int32, device=DEV)
    sr = _renderer(h)
    img, inv, radii = sr.render_cut(SC.faces(4), e32, e32, torch.empty(0, device=DEV), bg=SC.BG)
    torch.cuda.synchronize()
    assert tuple(radii.shape) == (4, 0) and sr.last_K == [0] * 4 and sr.last_kept == [0] * 4
    bg = torch.tensor(SC.BG, device=DEV).view(1, 3, 1, 1).expand(4, 3, SC.FACE, SC.FACE)
    assert torch.equal(img, bg) and int((inv != 0).sum()) == 0


# one wave, one wave exactly, a second wave, one past the compaction tile (256 rows), a ragged
# third tile; 65 537 rows would be the first with a second group of tiles: the 60 000-leaf cut is
# shorter, so the group prefix is exercised by test_second_group_of_tiles below
@pytest.mark.parametrize("R", [1, 63, 64, 65, 256, 257, 600])
def test_ragged_cut_lengths(R):
    h = SC.shell(DEV)
    ri, pi, w = SC.cut(DEV)
    # rows spread over the whole cut (and so over the sphere), in cut order
    pick = torch.linspace(0, ri.shape[0] - 1, R, device=DEV).long()
    _, _, radii, _ = _check(f"ragged_{R}", h, SC.faces(4), ri[pick].contiguous(), pi[pick].contiguous(),
                            w[pick].contiguous())
    if R >= 63:
        assert int((radii > 0).sum()) > 0


def test_second_group_of_tiles():
    """More than 256 tiles of 256 rows: the write launch adds the scanned group prefix.  The rows
    are the leaves themselves (the cut: every leaf, its tree parent, weight 1/2), sliced to one row
    past the first group."""
    h = SC.shell(DEV)
    nodes = h["nodes"]
    leaf = torch.nonzero(nodes[:, 3] > 0).flatten()[:256 * 256 + 1]
    if leaf.numel() < 256 * 256 + 1:  # 60 000 leaves: repeat rows to get past one group
        leaf = torch.cat([leaf, leaf[:256 * 256 + 1 - leaf.numel()]])
    ri = nodes[leaf, 2].contiguous()
    pi = nodes[nodes[leaf, 1].long(), 2].contiguous()
    w = torch.full((leaf.numel(),), 0.5, device=DEV)
    assert ri.shape[0] == 256 * 256 + 1
    _check("two_groups", h, SC.faces(4), ri, pi, w)


def test_cut_with_roots():
    """parent -1 reads the last row, as torch's gather does; with a weight below 1 the parent row
    contributes."""
    h = SC.shell(DEV, skybox=3000)
    ri, pi, w = (t.clone() for t in SC.cut(DEV, skybox=3000))
    rows = torch.arange(0, min(4000, ri.shape[0] - 3000), 37, device=DEV)
    pi[rows] = -1
    w[rows] = 0.5
    img, _, _, _ = _check("roots", h, SC.faces(4), ri, pi, w)
    ri0, pi0, w0 = SC.cut(DEV, skybox=3000)
    img0, _, _ = _renderer(h).render_cut(SC.faces(4), ri0, pi0, w0, bg=SC.BG)
    assert not torch.equal(img, img0)  # the changed rows are in view


def test_posed_station():
    """The centre off the origin and the rig rotated (posed_cases "mild"): the SH direction comes
    from campos, the view depth through view matrices that are no identity."""
    h = SC.shell(DEV, skybox=3000)
    rig, ctr = SC.mild_rig()
    assert float(np.abs(ctr).max()) > 0.2
    ri, pi, w = SC.cut(DEV, skybox=3000, center=tuple(float(x) for x in ctr))
    _check("posed_mild", h, SC.faces(6, center=ctr, rig=rig), ri, pi, w)


def test_view_depth_at_the_near_limit():
    """Leaves at view depth 0.2 and one float32 either side of it, on face 0's axis: the inputs say
    which side each lies on (station_cases.near_plane_leaves computes the depth on the host); only
    the one past 0.2 is kept and drawn."""
    tensors, sides = SC.near_plane_leaves(DEV)
    n = tensors["means3D"].shape[0]
    ri = torch.arange(n, dtype=torch.int32, device=DEV)
    w = torch.ones(n, device=DEV)
    cams = SC.faces(4)
    _, _, radii, sr = _check("near_limit", tensors, cams, ri, ri.clone(), w)
    src0 = set(sr.face_rows(0)["src"].tolist())
    assert 0 not in src0 and 1 not in src0 and 2 in src0
    assert radii[0, :3].tolist()[:2] == [0, 0] and int(radii[0, 2]) > 0
    assert all((i in src0) == bool(sides[i]) for i in range(3))
    # behind face 0 is in front of face 2 (it looks along -z) only when z < -0.2: none of the three
    assert not ({0, 1, 2} & set(sr.face_rows(2)["src"].tolist()))


def test_two_stations_in_turn_leave_no_state():
    h = SC.shell(DEV, skybox=3000)
    sr = _renderer(h)
    a_cams = SC.faces(6)
    b_cams = SC.faces(4, center=(0.8, -0.4, 1.1), rig=SC.yaw(30.0))
    a1 = sr.render(a_cams, SC.TAU, bg=SC.BG)
    a1 = tuple(t.clone() for t in a1)
    kept_a, K_a = list(sr.last_kept), list(sr.last_K)
    b = sr.render(b_cams, 2.0 * SC.TAU, bg=(0.0, 0.0, 0.0))
    assert list(sr.last_kept) != kept_a[:4]
    ri, pi, w = (t.clone() for t in sr.last_cut)
    _check("second_station", h, b_cams, ri, pi, w, sr=_renderer(h), bg=(0.0, 0.0, 0.0))
    fresh = _renderer(h).render_cut(b_cams, ri, pi, w, bg=(0.0, 0.0, 0.0))
    for x, y in zip(b, fresh):
        assert torch.equal(x, y)
    a2 = sr.render(a_cams, SC.TAU, bg=SC.BG)
    torch.cuda.synchronize()
    assert sr.last_kept == kept_a and sr.last_K == K_a
    for x, y in zip(a1, a2):
        assert torch.equal(x, y)


@pytest.mark.parametrize("D", [0, 1, 2])
def test_lower_sh_degrees(D):
    """Degree 3 is every other test's; 0 reads one float4 of each SH row and zeroes its tail."""
    h = SC.shell(DEV)
    ri, pi, w = SC.cut(DEV)
    _check(f"sh{D}", h, SC.faces(4)[1:3], ri, pi, w, D=D)


def test_mismatched_faces_and_too_many_are_refused():
    h = SC.shell(DEV)
    ri, pi, w = SC.cut(DEV)
    sr = _renderer(h)
    cams = SC.faces(4)
    with pytest.raises(ValueError, match="share W, H and tanfov"):
        sr.render_cut(cams[:1] + SC.faces(4, W=128)[1:2], ri, pi, w)
    with pytest.raises(RuntimeError, match="GSR_STATION_MAX_FACES"):
        sr.render_cut(cams + cams + cams[:1], ri, pi, w)
