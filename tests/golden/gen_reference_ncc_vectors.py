"""Generates tests/golden/reference_ncc.npz: the grey-image NCC term of the reference's OWN train_refreal.py calc_warp_loss
(get_consistency_loss2 over utils.loss_utils.lncc, and visual_refweight), lifted and run in float64 the way
gen_reference_warp_vectors.py does (whose lifting, namespace and camera stand-in are imported as they are), on the analytic two-view
scenes already stored in reference_warp.npz, with the cameras carrying the textured grey image of tests/multiview_ncc_statement.py and
rend_normal / rend_distance as leaves.  Recorded per case: what reference_warp.npz does not hold (the grey images, the scale of the
metal maps, the edge mask, the draw), ncc_loss (NaN where the reference returns None), its gradient into both maps and the
visual_refweight map.  Only inputs and outputs are committed; the reference source never travels.

    python tests/golden/gen_reference_ncc_vectors.py       # needs the reference checkout gen_reference_warp_vectors.py names
"""
import os
import random
from types import SimpleNamespace

import numpy as np
import torch

import gen_reference_warp_vectors as gw          # patches .cuda() / .float() and sets the default dtype to float64
import multiview_ncc_statement as mn

HERE = os.path.dirname(os.path.abspath(__file__))
W0 = np.load(os.path.join(HERE, "reference_warp.npz"))

CASES = {
    # name: (scene, iteration, k, seed, metal_scale, depth_scale_n, patch_size, keep_fraction)
    "ncc_8000": ("A", 8000, 400, 1, 1.0, 1.0, 3, 0.2),
    "ncc_15000": ("A", 15000, 400, 2, 1.0, 1.0, 3, 0.2),
    "ncc_all": ("A", 8000, 100000, 3, 1.0, 1.0, 3, 0.0),
    "ncc_ragged": ("B", 15000, 300, 4, 1.0, 1.0, 3, 0.2),
    "ncc_low_metal": ("A", 15000, 400, 5, 0.25, 1.0, 3, 0.0),
    "ncc_none_used": ("A", 15000, 400, 6, 8.0, 1.0, 3, 0.0),
    "ncc_no_valid": ("A", 8000, 400, 7, 1.0, 0.0, 3, 0.0),
    "ncc_patch1": ("A", 8000, 400, 8, 0.25, 1.0, 1, 0.0),
    "ncc_patch2": ("B", 15000, 300, 9, 0.25, 1.0, 2, 0.0),
}


def view(s, i):
    f = lambda k: torch.from_numpy(W0[f"{s}_{i}_{k}"])
    c = torch.from_numpy(W0[f"{s}_{i}_cam"])
    H, W = W0[f"{s}_{i}_depth"].shape
    cam = SimpleNamespace(image_width=W, image_height=H, FoVx=float(c[-2]), FoVy=float(c[-1]), world_view_transform=c[:16].reshape(4, 4).float(),
                          R=c[16:25].reshape(3, 3).float(), T=c[25:28].float())
    return SimpleNamespace(cam=cam, depth=f("depth"), normal=f("normal"), distance=f("distance"), base=f("base"), metal=f("metal"),
                           rough=f("rough"), fg=f("fg"))


def run(views, greys, case):
    v, n = views
    drawn = []
    ns = gw.namespace(case["keep"] == 0, drawn)
    gw.lift("train_refreal.py", ["calc_warp_loss", "visual_refweight", "get_consistency_loss2"], ns)
    g = {"torch": torch, "F": gw.F}
    gw.lift("scene/gaussian_model.py", ["get_points_depth_in_depth_map", "get_points_from_depth"], g, cls="GaussianModel")
    cmeth = {"torch": torch}
    gw.lift("scene/cameras.py", ["get_rays", "get_k", "get_inv_k", "get_image"], cmeth, cls="Camera")
    for k in ("get_rays", "get_k", "get_inv_k", "get_image"):
        setattr(gw.Cam, k, cmeth[k])
    gauss = SimpleNamespace(get_points_depth_in_depth_map=lambda *a, **k: g["get_points_depth_in_depth_map"](None, *a, **k),
                            get_points_from_depth=lambda *a, **k: g["get_points_from_depth"](None, *a, **k))
    cams, pkgs = [], []
    for i, x in enumerate((v, n)):
        cam = gw.Cam(x.cam, f"view{i}", greys[i].double()[None].expand(3, -1, -1))
        cam.original_image_gray = greys[i].double()[None]
        cams.append(cam)
        depth = x.depth * (case["depth_scale_n"] if i == 1 else 1.0)
        pk = {"surf_depth": depth[None].double(), "rend_normal": x.normal.double(), "rend_distance": x.distance[None].double(),
              "diffuse_map": x.base.double(), "refl_strength_map": x.metal[None].double() * case["metal_scale"],
              "roughness_map": x.rough[None].double()}
        pkgs.append(pk)
    leaves = [pkgs[0][k].clone().requires_grad_(True) for k in ("rend_normal", "rend_distance")]
    pkgs[0]["rend_normal"], pkgs[0]["rend_distance"] = leaves
    opt = SimpleNamespace(edge_aware_in_warp=True, use_virtul_cam=False, virtul_cam_prob=0.5, multi_view_patch_size=case["patch_size"],
                          multi_view_sample_num=case["k"], multi_view_pixel_noise_th=1.0, multi_view_ncc_weight=0.15, multi_view_geo_weight=0.03,
                          metallic_warp_weight=0.05, roughness_warp_weight=0.05, wo_use_geo_occ_aware=False, directional_rghmtl_warp_alignment=True,
                          srgb=False)
    scene = SimpleNamespace(getTrainCameras=lambda: [cams[1]])
    render = lambda cam, *a, **k: pkgs[1]
    mask_images = {"view0": v.fg.double()}
    np.random.seed(case["seed"])
    random.seed(0)
    out = ns["calc_warp_loss"](cams[0], scene, opt, gauss, SimpleNamespace(multi_view_max_dis=1.5, multi_view_max_angle=30), None, render,
                               pkgs[0], None, None, None, mask_images, case["iteration"], None, None, use_metallic_warp=True,
                               use_roughness_warp=True)
    ncc, refw = out[1], out[6]
    grads = [torch.zeros_like(l) for l in leaves]
    if ncc is not None and ncc.requires_grad:
        gr = torch.autograd.grad(ncc, leaves, allow_unused=True)
        grads = [torch.zeros_like(l) if x is None else x for l, x in zip(leaves, gr)]
    H, W = v.depth.shape
    return dict(ncc=np.nan if ncc is None else float(ncc), refw=refw.detach().numpy().reshape(H, W).astype(np.float32),
                g_normal=grads[0].detach().numpy().reshape(3, H, W).astype(np.float32),
                g_distance=grads[1].detach().numpy().reshape(H, W).astype(np.float32), drawn=None if not drawn else drawn[0],
                terms=[np.nan if t is None else float(t) for t in (out[0], out[2], out[3], out[4])])


def main():
    out = {}
    views, greys = {}, {}
    for s in ("A", "B"):
        views[s] = [view(s, 0), view(s, 1)]
        H, W = views[s][0].depth.shape
        greys[s] = mn.grey_pair(H, W)
        for i in (0, 1):
            out[f"{s}_{i}_grey"] = greys[s][i].numpy()
    for name, (s, it, k, seed, metal_scale, dscale, patch, keep_frac) in CASES.items():
        H, W = views[s][0].depth.shape
        keep = (torch.rand(H, W, generator=torch.Generator().manual_seed(seed)) >= keep_frac).to(torch.uint8)
        case = dict(iteration=it, k=k, seed=seed, metal_scale=metal_scale, depth_scale_n=dscale, patch_size=patch, keep=keep)
        r = run(views[s], greys[s], case)
        out[f"{name}_meta"] = np.array([it, k, metal_scale, dscale, patch], dtype=np.float64)
        out[f"{name}_scene"] = np.array(s)
        out[f"{name}_keep"] = np.packbits(keep.numpy())
        out[f"{name}_ncc"] = np.array(r["ncc"])
        out[f"{name}_terms"] = np.array(r["terms"])
        out[f"{name}_refw"] = r["refw"]
        out[f"{name}_g_normal"] = r["g_normal"]
        out[f"{name}_g_distance"] = r["g_distance"]
        if r["drawn"] is not None:
            out[f"{name}_drawn"] = r["drawn"].astype(np.int32)        # indices into the ascending list of valid pixels
        print(name, "ncc", r["ncc"], "drawn" if r["drawn"] is not None else "", "texels with a ref_weight", int((r["refw"] > 0).sum()),
              "gradient texels", int((r["g_distance"] != 0).sum()), "terms", r["terms"])
    path = os.path.join(HERE, "reference_ncc.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
