"""Generates tests/golden/reference_eval.npz by IMPORTING the reference's utils/loss_utils.py and utils/image_utils.py in the build
container and running its own ssim / psnr / l1_loss on seeded inputs, as eval.py:44-51 and train_refreal.py:1703-1704 call them.  Modules
the image lacks and this path never calls (kornia, cv2, lpips) are registered as empty placeholders so the import statements succeed; every
function that is executed is the reference's.  Only inputs and outputs are committed; the reference source never travels.

The images are smooth plus noise with a flat zero block and are left UNCLAMPED: about a fifth of the values lie outside [0, 1], so the
clamp of eval.py:44-46 matters.  Per shape the file holds, in float32 and in float64, after torch.clamp(., 0, 1): ssim, the whole-image
psnr (psnr on [1,3,H,W], eval.py:51), the per-channel-mean psnr (psnr(.).mean() on [3,H,W], train_refreal.py:1704) and l1.  For one depth
map per shape it holds the levels of visualize_depth's lines 75-76 (utils/image_utils.py) evaluated by numpy on the float32 map exactly
as written there; line 77 (cv2.applyColorMap) cannot run here and is left out.

    python tests/golden/gen_reference_eval_vectors.py       # needs /root/reference (absent on the GPU box)
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
sys.path.insert(0, REF)
for name in ("kornia", "kornia.filters", "cv2", "lpips"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["kornia.filters"].spatial_gradient = None
sys.modules["kornia"].filters = sys.modules["kornia.filters"]
from utils import image_utils, loss_utils  # noqa: E402

SHAPES = {"a": (37, 45), "b": (9, 70), "c": (64, 48), "d": (11, 11)}
out = {"window_2d": loss_utils.create_window(11, 3).numpy()[0, 0]}


def scene(H, W):
    g = torch.Generator().manual_seed(H * 1000 + W + 7)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = torch.stack([0.5 + 0.62 * torch.sin(6 * xx + 3 * yy), 0.5 + 0.62 * torch.cos(5 * yy + xx), 0.2 + 1.1 * xx * yy])
    gt = base + 0.06 * torch.randn(3, H, W, generator=g)
    gt[:, : max(1, H // 4), : max(1, W // 3)] = 0.0                    # flat background block (sigma = 0 region)
    img = gt + 0.1 * torch.randn(3, H, W, generator=g)
    img[:, : max(1, H // 8), : max(1, W // 6)] = 0.0                   # exact-equality region
    depth = 2.5 + 1.5 * torch.sin(4 * xx) * torch.cos(3 * yy) + 0.05 * torch.randn(H, W, generator=g)
    depth[: max(1, H // 4), : max(1, W // 3)] = 0.0                    # background: depth 0, the map's minimum many times over
    return img, gt, depth[None]


for tag, (H, W) in SHAPES.items():
    img, gt, depth = scene(H, W)
    outside = float(((img < 0) | (img > 1)).float().mean() + ((gt < 0) | (gt > 1)).float().mean()) / 2
    assert 0.12 < outside < 0.3, (tag, outside)
    out[f"{tag}_img"], out[f"{tag}_gt"], out[f"{tag}_depth"] = img.numpy(), gt.numpy(), depth.numpy()
    for dname, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        render_color = torch.clamp(img.to(dtype), 0.0, 1.0)                                  # eval.py:44-47
        gt_c = torch.clamp(gt.to(dtype), 0.0, 1.0)
        out[f"{tag}_{dname}_ssim"] = loss_utils.ssim(render_color[None], gt_c[None]).numpy()
        out[f"{tag}_{dname}_psnr_image"] = image_utils.psnr(render_color[None], gt_c[None]).numpy().reshape(())
        out[f"{tag}_{dname}_psnr_channels"] = image_utils.psnr(render_color, gt_c).mean().numpy()   # train_refreal.py:1704
        out[f"{tag}_{dname}_l1"] = loss_utils.l1_loss(render_color, gt_c).numpy()
    d = depth.detach().cpu().squeeze().numpy()                                               # utils/image_utils.py:74
    assert d.dtype == np.float32
    d = (d - d.min()) / (1e-20 + d.max() - d.min())                                          # :75
    assert d.dtype == np.float32, "numpy promoted the fp32 statement (needs numpy >= 2: python scalars are weak)"
    out[f"{tag}_depth_levels"] = (d * 255).clip(0, 255).astype(np.uint8)                     # :76
    print(tag, (H, W), f"outside [0,1]: {outside:.3f}", {k: float(out[f'{tag}_f64_{k}']) for k in ("ssim", "psnr_image", "psnr_channels", "l1")},
          "f32-f64:", {k: float(abs(out[f'{tag}_f32_{k}'].astype(np.float64) - out[f'{tag}_f64_{k}'])) for k in ("ssim", "psnr_image", "psnr_channels", "l1")})

dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_eval.npz")
np.savez_compressed(dst, **out)
print("wrote", dst, len(out), "arrays", os.path.getsize(dst), "bytes")
