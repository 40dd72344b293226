"""Generates tests/golden/reference_ref_score.npz by running the reference's OWN calc_ref_score and get_multi_view_neighbor -- the function
text of train_refreal.py (the same body in train_refnerf.py and train_glossy.py), with the two warp methods of scene/gaussian_model.py
and the camera methods of scene/cameras.py -- on four analytic views (tests/ref_score_statement.py: the two-view scene of
tests/multiview_statement.py at four azimuths, with photographs that carry a view-dependent lobe).  The recipe is that of
gen_reference_warp_vectors.py: the definitions are lifted out of the files with `ast` and executed in a namespace that holds what they
reference.  Stubs: tqdm is the identity, save_image / make_grid and os.makedirs do nothing (the function dumps debug PNGs),
dilated_edges_imgs returns ones (edges_aware = False: its result never reaches the return value), render_surfel returns the case's maps.
`.cuda()` is the identity and the default dtype is float64; unlike the warp script, `.float()` CASTS to float64 (the function feeds
integer torch.arange pixels through .float() into grid_sample).  So the reference runs in float64 on float32-rounded inputs and cameras.
Only inputs and outputs are committed; the reference source never travels.

    python tests/golden/gen_reference_ref_score_vectors.py <path of the reference checkout>
"""
import ast
import os
import sys
import types
from collections import defaultdict
from types import SimpleNamespace
from typing import List

import numpy as np
import torch
import torch.nn.functional as F

if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = sys.argv[1]
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
for name in ("kornia", "kornia.filters", "cv2", "lpips"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["kornia.filters"].spatial_gradient = None
sys.modules["kornia"].filters = sys.modules["kornia.filters"]
from utils import graphics_utils  # noqa: E402  (the reference's)

import ref_score_statement as rs  # noqa: E402   (the analytic views only)

torch.Tensor.cuda = lambda self, *a, **k: self
torch.Tensor.float = lambda self, *a, **k: self.to(torch.float64)
torch.set_default_dtype(torch.float64)

H, W, AZ = 40, 52, (30.0, 37.0, 24.0, 41.0)


def lift(path, names, ns, cls=None):
    """exec the top-level functions `names` of `path` (or the methods of class `cls`) in `ns`."""
    tree = ast.parse(open(os.path.join(REF, path)).read())
    body = tree.body
    if cls is not None:
        body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    for node in body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    missing = [n for n in names if n not in ns]
    assert not missing, missing


class Cam:
    def __init__(self, view):
        mini = view.cam
        self.image_width, self.image_height, self.image_name = mini.image_width, mini.image_height, view.name
        self.world_view_transform = mini.world_view_transform.double()
        self.camera_center = mini.camera_center.double()
        self.R, self.T = mini.R.double(), mini.T.double()
        self.Fx, self.Fy, self.Cx, self.Cy = rs.intrinsics(mini)
        self.original_image = view.image.double()
        self.original_image_gray = self.original_image.mean(0, keepdim=True)


def main():
    views = rs.analytic_views(H, W, AZ)
    pkgs = {v.name: {"surf_depth": v.depth[None].double(), "rend_normal": v.normal.double(), "rend_distance": v.distance[None].double()}
            for v in views}
    ns = {"torch": torch, "F": F, "np": np, "defaultdict": defaultdict, "List": List, "tqdm": lambda it, **k: it,
          "save_image": lambda *a, **k: None, "make_grid": lambda t, **k: t, "os": SimpleNamespace(makedirs=lambda *a, **k: None),
          "dilated_edges_imgs": lambda img, dilate_size=2: torch.ones(H, W),
          "render_surfel": lambda cam, *a, **k: pkgs[cam.image_name],
          "patch_offsets": graphics_utils.patch_offsets, "patch_warp": graphics_utils.patch_warp,
          "Camera": object, "Scene": object, "OptimizationParams": object, "GaussianModel": object, "ModelParams": object,
          "PipelineParams": object, "print": lambda *a, **k: None}
    lift("train_refreal.py", ["calc_ref_score", "get_multi_view_neighbor"], ns)
    g = {"torch": torch, "F": F}
    lift("scene/gaussian_model.py", ["get_points_depth_in_depth_map", "get_points_from_depth"], g, cls="GaussianModel")
    cmeth = {"torch": torch}
    lift("scene/cameras.py", ["get_rays", "get_k", "get_inv_k", "get_image"], cmeth, cls="Camera")
    for k in ("get_rays", "get_k", "get_inv_k", "get_image"):
        setattr(Cam, k, cmeth[k])
    gauss = SimpleNamespace(get_points_depth_in_depth_map=lambda *a, **k: g["get_points_depth_in_depth_map"](None, *a, **k),
                            get_points_from_depth=lambda *a, **k: g["get_points_from_depth"](None, *a, **k))
    cams = [Cam(v) for v in views]
    scene = SimpleNamespace(getTrainCameras=lambda: cams)
    opt = SimpleNamespace(srgb=False, multi_view_pixel_noise_th=1.0)
    lists = ns["get_multi_view_neighbor"](scene)
    scores = ns["calc_ref_score"](scene, opt, gauss, None, None, None, None, None, None, 0, None)
    out = {"az": np.array(AZ), "th": np.array(opt.multi_view_pixel_noise_th)}
    nb = np.full((len(views), 20), -1, dtype=np.int32)
    for i, v in enumerate(views):
        for k in ("depth", "normal", "distance", "image"):
            out[f"{i}_{k}"] = getattr(v, k).numpy()
        c = v.cam
        out[f"{i}_cam"] = np.concatenate([c.world_view_transform.numpy().reshape(-1), c.R.numpy().reshape(-1), c.T.numpy().reshape(-1),
                                          c.camera_center.numpy().reshape(-1), [c.FoVx, c.FoVy]]).astype(np.float64)
        ids = [idx for idx, _name in lists[v.name]]
        nb[i, :len(ids)] = ids
        out[f"{i}_score"] = scores[v.name].reshape(H, W).numpy().astype(np.float64)
        print(v.name, "neighbours", ids, "max", float(scores[v.name].max()), "covered", float((scores[v.name] > 0).double().mean()))
    out["neighbours"] = nb
    path = os.path.join(HERE, "reference_ref_score.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
