"""Generates tests/golden/reference_mesh_colour.npz by running the reference's OWN compute_unbounded_tsdf(..., return_rgb=True) over
compute_sdf_perframe -- the two function texts nested inside GaussianExtractor.extract_mesh_unbounded (utils/mesh_utils.py:322-373),
lifted out of the file with `ast` because the module imports Open3D, trimesh and the CUDA stack at its top -- on three analytic views of
the sphere-and-wall scene of tests/mesh_statement.py.  They are executed in a namespace where `self` is a SimpleNamespace(viewpoint_stack,
depthmaps, rgbmaps), `tqdm` is the identity, `.cuda()` is the identity and the default dtype is float64, so the reference runs in float64
on inputs that are exact in float32.  inv_contraction is None, as in the texturing call (:402); voxel_size = 0.02, so trunc = 0.1.

Recorded: the inputs (projection matrices, depth maps, rgb maps, points, all float32) and the returned tsdfs / rgbs (float64).  Only data
is committed; the reference source never travels.

    python tests/golden/gen_reference_mesh_colour_vectors.py <path of the reference tree>
"""
import ast
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import mesh_attr_statement as mas  # noqa: E402   (the analytic maps only)
import mesh_statement as ms  # noqa: E402

VIEWS = ((20, 24, 10.0, 0.0), (28, 32, 130.0, 20.0), (20, 24, 250.0, -35.0))      # H, W, azimuth, elevation
N_POINTS, VOXEL = 257, 0.02


def lift_nested(ref, path, cls, method, names, ns):
    """exec the functions `names` defined inside `cls.method` of `path` in `ns`."""
    tree = ast.parse(open(os.path.join(ref, path)).read())
    body = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    fn = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == method)
    for node in fn.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    missing = [n for n in names if n not in ns]
    assert not missing, missing


def main():
    from materialrefgs_amd.camera import look_at_camera
    ref = sys.argv[1]
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.set_default_dtype(torch.float64)
    out = {}
    cams, depthmaps, rgbmaps = [], [], []
    for i, (H, W, az, el) in enumerate(VIEWS):
        cam = look_at_camera(az, el, 2.2, math.radians(40.0), H, W)
        proj = cam.full_proj_transform.numpy().astype(np.float32)
        depth = ms.analytic_depth(cam, H, W)
        rgb = mas.analytic_attributes(i, H, W, 3)
        out[f"proj_{i}"], out[f"depth_{i}"], out[f"rgb_{i}"] = proj, depth, rgb
        cams.append(SimpleNamespace(full_proj_transform=torch.from_numpy(proj).double()))
        depthmaps.append(torch.from_numpy(depth).double()[None])
        rgbmaps.append(torch.from_numpy(rgb).double().permute(2, 0, 1).contiguous())
    rng = np.random.default_rng(7)
    d = rng.standard_normal((N_POINTS, 3))
    pts = (d / np.linalg.norm(d, axis=1, keepdims=True) * (0.5 + rng.uniform(-0.03, 0.03, (N_POINTS, 1)))).astype(np.float32)
    out["points"] = pts
    ns = {"torch": torch, "tqdm": lambda it, **k: it, "self": SimpleNamespace(viewpoint_stack=cams, depthmaps=depthmaps, rgbmaps=rgbmaps)}
    lift_nested(ref, "utils/mesh_utils.py", "GaussianExtractor", "extract_mesh_unbounded", ["compute_sdf_perframe", "compute_unbounded_tsdf"], ns)
    tsdfs, rgbs = ns["compute_unbounded_tsdf"](torch.from_numpy(pts).double(), inv_contraction=None, voxel_size=VOXEL, return_rgb=True)
    out["voxel_size"] = np.array(VOXEL)
    out["tsdfs"], out["rgbs"] = tsdfs.numpy().astype(np.float64), rgbs.numpy().astype(np.float64)
    path = os.path.join(HERE, "reference_mesh_colour.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; coloured points", int((out["rgbs"] != 0).any(axis=1).sum()), "of", N_POINTS)


if __name__ == "__main__":
    main()
