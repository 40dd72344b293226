"""Generates tests/golden/reference_lpips.npz by IMPORTING the reference's lpipsPyTorch package in the build container and running its own
LPIPS.forward, BaseNet.forward and normalize_activation (+ torch.autograd) in float64 on seeded images.  torchvision is absent here and
the weights are downloads, so `torchvision.models.vgg16(...).features` is a stand-in: the 31-module sequence of VGG16's features with the
seeded weights of materialrefgs_amd.lpips.random_weights, and get_state_dict is stubbed with the same generator's lin vectors.  Every
function that is executed on the images is the reference's.  Only images, seeds, outputs and dx are committed, never the 59 MB of weights;
the reference source never travels.

    python tests/golden/gen_reference_lpips_vectors.py       # needs /root/reference (absent on the GPU box)
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)                                   # the reference's lpipsPyTorch, not this repository's shim of the same name
from materialrefgs_amd.lpips import CONV_INDEX, random_weights  # noqa: E402

SEED = 0
conv_w, conv_b, lin_w = random_weights(SEED)


def vgg16(*a, **k):
    cfg = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
    layers, cin = [], 3
    for v in cfg:
        if v == "M":
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    features = nn.Sequential(*layers)
    assert len(features) == 31
    for i, n in enumerate(CONV_INDEX):
        features[n].weight.data.copy_(conv_w[i])
        features[n].bias.data.copy_(conv_b[i])
    return types.SimpleNamespace(features=features)


tv = types.ModuleType("torchvision")
tv.models = types.ModuleType("torchvision.models")
tv.models.vgg16 = vgg16
tv.models.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1=None)
sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, tv.models
from lpipsPyTorch.modules import lpips as ref_lpips  # noqa: E402
assert ref_lpips.__file__.startswith(REF)
ref_lpips.get_state_dict = lambda net_type, version: {f"{k}.1.weight": w.reshape(1, -1, 1, 1) for k, w in enumerate(lin_w)}

criterion = ref_lpips.LPIPS("vgg").double()
out = {"seed": np.int64(SEED)}
for tag, (H, W) in {"a": (16, 16), "b": (19, 22), "c": (24, 17)}.items():
    g = torch.Generator().manual_seed(1000 * H + W)
    x = (torch.rand(1, 3, H, W, generator=g) * 2 - 1).float()
    y = (torch.rand(1, 3, H, W, generator=g) * 2 - 1).float()
    xd = x.double().requires_grad_(True)
    d = criterion(xd, y.double())
    dx, = torch.autograd.grad(d.sum(), xd)
    assert bool(torch.isfinite(dx).all())
    feats = criterion.net(x.double())                     # BaseNet.forward: the five normalised taps
    out[f"{tag}_x"], out[f"{tag}_y"] = x[0].numpy(), y[0].numpy()
    out[f"{tag}_out"], out[f"{tag}_dx"] = d.detach().numpy(), dx[0].numpy()
    out[f"{tag}_feat5"] = feats[4].detach()[0].numpy()
    out[f"{tag}_feat1_norm"] = feats[0].detach()[0].pow(2).sum(0).numpy()
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_lpips.npz"), **out)
print({k: getattr(v, "shape", v) for k, v in out.items()})
