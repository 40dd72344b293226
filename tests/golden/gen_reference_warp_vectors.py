"""Generates tests/golden/reference_warp.npz by running the reference's OWN calc_warp_loss -- the function text of train_refnerf.py
(same body as train_glossy.py) and of train_refreal.py, with its helpers visual_refweight / get_consistency_loss2, the two warp methods
of scene/gaussian_model.py and the camera methods of scene/cameras.py -- on the analytic two-view scene of tests/multiview_statement.py.
The training scripts import the whole CUDA stack at module level, so the definitions are lifted out of the files with `ast` and executed
in a namespace that holds what they reference: torch, F, numpy, random, the reference's own utils.graphics_utils (patch_offsets,
patch_warp) and utils.loss_utils (lncc; kornia / cv2 / lpips are empty placeholders, as in gen_reference_loss_vectors.py).
dilated_edges_imgs (cv2 Canny) is replaced by the case's edge mask and np.random.choice is wrapped to record the draw.  `.cuda()` is the
identity, `.float()` too and the default dtype is float64, so the reference runs in float64 on float32-rounded inputs and cameras.
Only inputs and outputs are committed; the reference source never travels.

    python tests/golden/gen_reference_warp_vectors.py       # needs /root/reference (absent on the GPU box)
"""
import ast
import os
import random
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
for name in ("kornia", "kornia.filters", "cv2", "lpips"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["kornia.filters"].spatial_gradient = None
sys.modules["kornia"].filters = sys.modules["kornia.filters"]
from utils import graphics_utils, loss_utils  # noqa: E402  (the reference's)

import multiview_statement as ms  # noqa: E402   (the analytic scene only)

torch.Tensor.cuda = lambda self, *a, **k: self
torch.Tensor.float = lambda self, *a, **k: self
torch.set_default_dtype(torch.float64)


def lift(path, names, ns, cls=None):
    """exec the top-level functions `names` of `path` (or the methods of class `cls`) in `ns`."""
    src = open(os.path.join(REF, path)).read()
    tree = ast.parse(src)
    body = tree.body
    if cls is not None:
        body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    for node in body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    missing = [n for n in names if n not in ns]
    assert not missing, missing


def namespace(edge_mask, drawn):
    ns = {"torch": torch, "F": F, "np": SimpleNamespace(random=SimpleNamespace(random=np.random.random, choice=None)), "random": random,
          "patch_offsets": graphics_utils.patch_offsets, "patch_warp": graphics_utils.patch_warp, "lncc": loss_utils.lncc,
          "gen_virtul_cam": None, "Camera": object, "Scene": object, "OptimizationParams": object, "GaussianModel": object,
          "ModelParams": object, "PipelineParams": object,
          "dilated_edges_imgs": lambda img, dilate_size=7: edge_mask.to(torch.float64)}

    def choice(n, k, replace=True):
        idx = np.random.choice(n, k, replace=replace)
        drawn.append(idx.copy())
        return idx
    ns["np"].random.choice = choice
    return ns


class Cam:
    def __init__(self, mini, name, img):
        W, H = mini.image_width, mini.image_height
        self.image_width, self.image_height, self.image_name = W, H, name
        self.world_view_transform = mini.world_view_transform.double()
        self.R, self.T = mini.R.double(), mini.T.double()
        self.Fx, self.Fy, self.Cx, self.Cy = ms_intr(mini)
        self.ncc_scale = 1.0
        self.nearest_id = [0]
        self.original_image = img
        self.original_image_gray = (0.299 * img[0] + 0.587 * img[1] + 0.114 * img[2])[None]
        self.HWK = (H, W, None)


def ms_intr(cam):
    from materialrefgs_amd.camera import fov2focal
    W, H = cam.image_width, cam.image_height
    return tuple(float(np.float32(x)) for x in (fov2focal(cam.FoVx, W), fov2focal(cam.FoVy, H), 0.5 * W, 0.5 * H))


MAPS = ("surf_depth", "diffuse_map", "refl_strength_map", "roughness_map")


def run(script, views, case):
    v, n = views
    drawn = []
    ns = namespace(case["keep"] == 0, drawn)
    lift(script, ["calc_warp_loss", "visual_refweight"] + (["get_consistency_loss2"] if "refreal" in script else []), ns)
    g = {"torch": torch, "F": F}
    lift("scene/gaussian_model.py", ["get_points_depth_in_depth_map", "get_points_from_depth"], g, cls="GaussianModel")
    cmeth = {"torch": torch}
    lift("scene/cameras.py", ["get_rays", "get_k", "get_inv_k", "get_image"], cmeth, cls="Camera")
    for k in ("get_rays", "get_k", "get_inv_k", "get_image"):
        setattr(Cam, k, cmeth[k])
    gauss = SimpleNamespace(get_points_depth_in_depth_map=lambda *a, **k: g["get_points_depth_in_depth_map"](None, *a, **k),
                            get_points_from_depth=lambda *a, **k: g["get_points_from_depth"](None, *a, **k))
    gen = torch.Generator().manual_seed(11)
    cams, pkgs, leaves = [], [], []
    for i, x in enumerate((v, n)):
        img = torch.rand(3, x.depth.shape[0], x.depth.shape[1], generator=gen)
        cams.append(Cam(x.cam, f"view{i}", img))
        depth = x.depth * (case["depth_scale_n"] if i == 1 else 1.0)
        pk = {"surf_depth": depth[None].double(), "rend_normal": x.normal.double(), "rend_distance": x.distance[None].double() * case["dist_scale"],
              "diffuse_map": x.base.double(), "refl_strength_map": x.metal[None].double(), "roughness_map": x.rough[None].double()}
        for k in MAPS:
            pk[k] = pk[k].clone().requires_grad_(True)
        leaves += [pk[k] for k in MAPS]
        pkgs.append(pk)
    opt = SimpleNamespace(edge_aware_in_warp=True, use_virtul_cam=False, virtul_cam_prob=0.5, multi_view_patch_size=3,
                          multi_view_sample_num=case["k"], multi_view_pixel_noise_th=1.0, multi_view_ncc_weight=0.15, multi_view_geo_weight=0.03,
                          metallic_warp_weight=0.05, roughness_warp_weight=0.05, wo_use_geo_occ_aware=False, directional_rghmtl_warp_alignment=True,
                          srgb=False)
    scene = SimpleNamespace(getTrainCameras=lambda: [cams[1]])
    render = lambda cam, *a, **k: pkgs[1]
    mask_images = {"view0": (v.fg * case["fg_scale"]).double()}
    np.random.seed(case["seed"])
    random.seed(0)
    out = ns["calc_warp_loss"](cams[0], scene, opt, gauss, SimpleNamespace(multi_view_max_dis=1.5, multi_view_max_angle=30), None, render,
                               pkgs[0], None, None, None, mask_images, case["iteration"], None, None, use_metallic_warp=True,
                               use_roughness_warp=True)
    geo, ncc, base, metal, rough, weight = out[:6]
    terms = [geo, base, metal, rough]
    up = [0.7, 1.3, 0.9, 1.1]
    live = [(t, u) for t, u in zip(terms, up) if t is not None and t.requires_grad and torch.isfinite(t)]
    grads = [torch.zeros_like(l) for l in leaves]
    if live:
        gr = torch.autograd.grad(sum(t * u for t, u in live), leaves, allow_unused=True)
        grads = [torch.zeros_like(l) if x is None else x for l, x in zip(leaves, gr)]
    return dict(terms=np.array([np.nan if t is None else float(t) for t in terms]),
                present=np.array([t is not None for t in terms]), weight=weight.detach().numpy().reshape(v.depth.shape),
                ncc=np.nan if ncc is None else float(ncc), grads=[x.detach().reshape(-1, *v.depth.shape).squeeze(0).numpy().astype(np.float32) for x in grads],
                drawn=None if not drawn else drawn[0])


CASES = {
    # name: (scene, script, iteration, k, seed, fg_scale, depth_scale_n, dist_scale, keep_fraction)
    "refnerf_all": ("A", "train_refnerf.py", 30000, 100000, 1, 1.0, 1.0, 1.0, 0.0),
    "refnerf_draw": ("A", "train_refnerf.py", 30000, 150, 2, 1.0, 1.0, 1.0, 0.2),
    "ragged_draw": ("B", "train_refnerf.py", 30000, 200, 3, 1.0, 1.0, 1.0, 0.2),
    "refreal_15000": ("A", "train_refreal.py", 15000, 150, 4, 1.0, 1.0, 1.0, 0.2),
    "refreal_8000": ("A", "train_refreal.py", 8000, 150, 5, 1.0, 1.0, 1.0, 0.2),
    "empty_keep": ("A", "train_refnerf.py", 30000, 150, 6, 0.5, 1.0, 1.0, 0.0),
    "no_valid": ("A", "train_refreal.py", 30000, 150, 7, 1.0, 0.0, 1.0, 0.0),
}
SCENES = {"A": (32, 40), "B": (29, 37)}


def main():
    out = {}
    views = {}
    for s, (H, W) in SCENES.items():
        views[s] = ms.analytic_pair(H, W)
        for i, x in enumerate(views[s]):
            for k in ("depth", "normal", "distance", "base", "metal", "rough", "fg"):
                out[f"{s}_{i}_{k}"] = getattr(x, k).numpy()
            out[f"{s}_{i}_cam"] = np.concatenate([x.cam.world_view_transform.numpy().reshape(-1), x.cam.R.numpy().reshape(-1),
                                                  x.cam.T.numpy().reshape(-1), [x.cam.FoVx, x.cam.FoVy]]).astype(np.float64)
    for name, (s, script, it, k, seed, fg_scale, dscale, dist_scale, keep_frac) in CASES.items():
        H, W = SCENES[s]
        keep = (torch.rand(H, W, generator=torch.Generator().manual_seed(seed)) >= keep_frac).to(torch.uint8)
        case = dict(iteration=it, k=k, seed=seed, fg_scale=fg_scale, depth_scale_n=dscale, dist_scale=dist_scale, keep=keep)
        r = run(script, views[s], case)
        meta = np.array([it, k, fg_scale, dscale, dist_scale, 1.0 if "refreal" in script else 0.0], dtype=np.float64)
        out[f"{name}_meta"] = meta
        out[f"{name}_scene"] = np.array(s)
        out[f"{name}_keep"] = keep.numpy()
        out[f"{name}_terms"] = r["terms"]
        out[f"{name}_present"] = r["present"]
        out[f"{name}_weight"] = r["weight"]
        if r["drawn"] is not None:
            out[f"{name}_drawn"] = r["drawn"].astype(np.int32)        # indices into the ascending list of valid pixels
        for i, (who, key) in enumerate([(w, m) for w in ("v", "n") for m in MAPS]):
            out[f"{name}_g_{who}_{key}"] = r["grads"][i]
        print(name, r["terms"], "drawn" if r["drawn"] is not None else "", "ncc", r["ncc"])
    path = os.path.join(HERE, "reference_warp.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
