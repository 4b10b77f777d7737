"""Generate tests/golden/lpips.npz from the reference's own LPIPS module (build container only, CPU).

The reference's lpipsPyTorch is imported with torchvision.models and
torch.hub.load_state_dict_from_url stubbed to hand it the tensors of tests/lpips_ref.make_weights(0)
instead of the trained weights (59 MB, fetched from the network by the reference): a VGG16-shaped
`features` stack built here, and the five linear layers under the weight file's key names.  The code
that runs is the reference's LPIPS.forward (modules/lpips.py, networks.py, utils.py).

Cases: 16x16 (stage five is 1x1), 37x53 (odd sizes, floor pooling) and 106x159 (torch's fp32 nearest
rule differs from the integer rule at stage three on both axes).  Per case: two unclamped noisy
images, an alpha mask with a hole, and five regions as bits 0..4 -- all ones, empty, the single pixel
(5, 7), and two overlapping blobs.  Stored per case: the inputs, the bits, and for row 0 (no mask) and
each region what LPIPS.forward returns on (clamp(image) alpha, clamp(gt) alpha) -- the total and its
five per-stage terms (the list the forward concatenates) -- in fp32 (`ref32`, `stages32`) and with the
module and the inputs cast to fp64 (`ref64`, `stages64`).

D_whole / D_region / D_single: the largest |ref32 - ref64| over the cases for row 0, the all-ones and
blob regions, and the one-pixel region: the reference's own fp32 error, from which the tests take
their tolerances.  `weight_names`, `weight_sums`: every generated weight tensor's fp64 sum and sum of
squares, so a drift of the generator fails loudly.

Nothing from the reference is copied; only numbers are kept.
Usage:  python tests/golden/make_lpips_golden.py --ref <reference checkout>
"""
from __future__ import annotations

import argparse
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import lpips_ref  # noqa: E402

SIZES = [(16, 16), (37, 53), (106, 159)]
KINDS = ["whole", "region", "empty", "single", "region", "region"]


def vgg16_features(vgg):
    """torchvision's vgg16().features layout (configuration D) holding the given tensors."""
    layers, cin = [], 3
    for k, (convs, c) in enumerate(zip(lpips_ref.STAGE_CONVS, lpips_ref.STAGE_CHANNELS)):
        for _ in convs:
            layers += [nn.Conv2d(cin, c, 3, padding=1), nn.ReLU(inplace=True)]
            cin = c
        layers.append(nn.MaxPool2d(2, 2))
    seq = nn.Sequential(*layers)
    seq.load_state_dict({k[len("features."):]: v for k, v in vgg.items()})
    return seq


def import_reference(ref, vgg, lin):
    models = types.ModuleType("torchvision.models")
    models.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1=None)
    models.vgg16 = lambda weights=None: types.SimpleNamespace(features=vgg16_features(vgg))
    tv = types.ModuleType("torchvision")
    tv.models = models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models
    torch.hub.load_state_dict_from_url = lambda url, **kw: dict(lin)
    sys.path.insert(0, ref)
    import lpipsPyTorch
    import lpipsPyTorch.modules.lpips as mod

    class Spy:  # records the per-stage list the forward concatenates
        def __getattr__(self, name):
            return getattr(torch, name)

        def cat(self, tensors, dim=0):
            self.stages = [float(t.reshape(())) for t in tensors]
            return torch.cat(tensors, dim)

    mod.torch = spy = Spy()
    return lpipsPyTorch.modules.lpips.LPIPS("vgg"), spy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout")
    vgg, lin = lpips_ref.make_weights(0)
    model, spy = import_reference(ap.parse_args().ref, vgg, lin)
    model32, model64 = model.eval(), None
    import copy
    model64 = copy.deepcopy(model).double().eval()
    names, sums = lpips_ref.weight_checksums(vgg, lin)
    out = {"n": np.int32(len(SIZES)), "weight_names": np.array(names), "weight_sums": sums,
           "kinds": np.array(KINDS)}
    D = {"whole": 0.0, "region": 0.0, "single": 0.0}
    g = torch.Generator().manual_seed(31)
    for k, (H, W) in enumerate(SIZES):
        raw = torch.rand((3, H, W), generator=g) * 1.3 - 0.15  # some values outside [0, 1]
        raw_gt = raw + 0.1 * torch.randn((3, H, W), generator=g)
        alpha = torch.ones((1, H, W))
        alpha[:, H // 4:H // 4 + max(2, H // 5), W // 2:W // 2 + max(2, W // 4)] = 0.0  # the hole
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        blob = lambda cy, cx, r: (((yy - cy * H) ** 2 + (xx - cx * W) ** 2) < (r * min(H, W)) ** 2).float()
        single = torch.zeros((H, W))
        single[5, 7] = 1.0
        masks = [torch.ones((H, W)), torch.zeros((H, W)), single, blob(0.4, 0.35, 0.33), blob(0.6, 0.6, 0.3)]
        assert (masks[3] * masks[4]).sum() > 0 and alpha[0, 5, 7] == 1
        x, y = lpips_ref.masked_inputs(raw, raw_gt, alpha)
        ref, stages = {}, {}
        for tag, m, cast in (("32", model32, lambda t: t), ("64", model64, lambda t: t.double())):
            tot, st = [], []
            with torch.no_grad():
                for mask in [None] + masks:
                    v = m(cast(x), cast(y), None if mask is None else cast(mask)[None])
                    tot.append(float(v.reshape(())))
                    st.append(list(spy.stages))
            ref[tag], stages[tag] = np.array(tot, np.float64), np.array(st, np.float64).T  # (5, rows)
        assert np.isfinite(ref["64"]).all() and ref["64"][2] == 0.0 and ref["64"][0] > 0.01
        assert stages["64"][1:, 3].max() == 0.0 < stages["64"][0, 3]  # the pixel is dropped below stage one
        for r, kind in enumerate(KINDS):
            if kind in D:
                D[kind] = max(D[kind], abs(ref["32"][r] - ref["64"][r]))
        bits = torch.zeros((H, W), dtype=torch.int32)
        for r, m in enumerate(masks):
            bits |= m.to(torch.int32) << r
        out.update({f"image_{k}": raw.numpy(), f"gt_{k}": raw_gt.numpy(), f"alpha_{k}": alpha[0].numpy(),
                    f"bits_{k}": bits.numpy().astype(np.uint16), f"ref32_{k}": ref["32"], f"ref64_{k}": ref["64"],
                    f"stages32_{k}": stages["32"], f"stages64_{k}": stages["64"]})
    for kind, v in D.items():
        out["D_" + kind] = np.float64(v)
    path = os.path.join(OUT, "lpips.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1_000_000
    print(f"{path}: {os.path.getsize(path)} bytes; D {D}; whole-image values "
          f"{[float(out[f'ref64_{k}'][0]) for k in range(len(SIZES))]}")


if __name__ == "__main__":
    main()
