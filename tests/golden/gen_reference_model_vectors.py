"""Generates tests/golden/reference_model.npz by running the reference's OWN GaussianModel (scene/gaussian_model.py) on the CPU in its
native float32: the class definition and the two get_env_direction functions are lifted out of the file with `ast` (the module itself
imports the CUDA stack at the top) and executed in a namespace that holds what they reference -- torch, numpy and the reference's own
utils.general_utils / utils.graphics_utils helpers.  `.cuda()` is the identity and every device argument naming cuda names the CPU.

Recorded (data only; the reference source never travels):
  * the reset family on the P = 64 model of tests/model_statement.random_model (raw values in [-6, 6], resampled there until every decision
    keeps a relative margin of 1e-3 -- asserted here again, no row is left out): the new raw tensor of every covered method, with and
    without the exclusive mask where the method takes one, and the three sequences the training loops run.  torch.rand_like is REPLACED
    by the statement's recorded uniforms (`u_f_dc`, `u_ori_color`), so the drawing methods are compared element by element.
    The reference's replace_tensor_to_optimizer does nothing for a group without optimizer state, so every group is given one first.
  * get_env_direction1 / 2 at H = 8, W = 16
  * get_normal(return_delta=True) at P = 16 with its inputs
  * the attribute names behind the entries of capture(), in order

    python tests/golden/gen_reference_model_vectors.py       # needs /root/reference (absent on the GPU box)
"""
import ast
import os
import sys

import numpy as np
import torch
from torch import nn

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
from utils import general_utils, graphics_utils  # noqa: E402  (the reference's)

import model_statement as ms  # noqa: E402

P, SEED = 64, 20
_GIVEN_UNIFORMS = []           # what the next torch.rand_like calls return


def _cpu(v):
    if isinstance(v, str) and v.startswith("cuda"):
        return "cpu"
    if isinstance(v, torch.device) and v.type == "cuda":
        return torch.device("cpu")
    return v


class _CudaIsCpu(torch.overrides.TorchFunctionMode):
    def __torch_function__(self, func, types_, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        if name == "cuda" and args and isinstance(args[0], torch.Tensor):
            return args[0]
        if name == "rand_like":
            u = _GIVEN_UNIFORMS.pop(0)
            assert u.shape == args[0].shape and u.dtype == args[0].dtype
            return u.clone()
        return func(*[_cpu(a) for a in args], **{k: _cpu(v) for k, v in kwargs.items()})


def lift_class():
    tree = ast.parse(open(os.path.join(REF, "scene", "gaussian_model.py")).read())
    keep = [n for n in tree.body if (isinstance(n, ast.FunctionDef) and n.name.startswith("get_env_direction")) or
            (isinstance(n, ast.ClassDef) and n.name == "GaussianModel")]
    assert len(keep) == 3
    ns = {"torch": torch, "np": np, "nn": nn, "os": os, "BasicPointCloud": graphics_utils.BasicPointCloud,
          "init_predefined_omega": graphics_utils.init_predefined_omega}
    for name in ("inverse_sigmoid", "get_expon_lr_func", "build_rotation", "strip_symmetric", "build_scaling_rotation", "safe_normalize",
                 "flip_align_view"):
        ns[name] = getattr(general_utils, name)
    exec(compile(ast.Module(body=keep, type_ignores=[]), "scene/gaussian_model.py", "exec"), ns)
    return ns


GROUP_ATTRS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
               "rotation": "_rotation", "refl_strength": "_refl_strength", "ori_color": "_ori_color", "diffuse_color": "_diffuse_color",
               "roughness": "_roughness", "metalness": "_metalness", "normal1": "_normal1", "normal2": "_normal2", "ind_dc": "_indirect_dc",
               "ind_rest": "_indirect_rest", "ind_asg": "_indirect_asg"}
SHAPES = {"xyz": (3,), "rotation": (4,), "diffuse_color": (3,), "metalness": (1,), "normal1": (3,), "normal2": (3,), "ind_dc": (1, 3),
          "ind_rest": (15, 3), "ind_asg": (32, 5)}


def make(cls, model, n=P):
    """A reference model holding the statement's model, with a stepped Adam over the sixteen per-gaussian groups."""
    g = torch.Generator().manual_seed(3)
    m = cls(3)
    for name, attr in GROUP_ATTRS.items():
        t = torch.from_numpy(model[name].astype(np.float32)) if name in model else torch.randn((n,) + SHAPES[name], generator=g)
        setattr(m, attr, nn.Parameter(t.clone().requires_grad_(True)))
    for k in ms.SETTINGS:
        setattr(m, k, model[k])
    m.optimizer = torch.optim.Adam([{"params": [getattr(m, a)], "lr": 1e-3, "name": k} for k, a in GROUP_ATTRS.items()], lr=0.0, eps=1e-15)
    for grp in m.optimizer.param_groups:
        p = grp["params"][0]
        m.optimizer.state[p] = {"step": torch.tensor(5.0), "exp_avg": torch.ones_like(p), "exp_avg_sq": torch.ones_like(p)}
    return m


def main():
    ns = lift_class()
    cls = ns["GaussianModel"]
    out = {}
    with _CudaIsCpu():
        model, exclusive, u = ms.random_model(P, SEED)
        excl = torch.from_numpy(exclusive)
        for k in ms.GROUPS:
            out[f"in_{k}"] = model[k].astype(np.float32)
        out["in_exclusive"] = exclusive
        out["u_f_dc"], out["u_ori_color"] = u["f_dc"].astype(np.float32), u["ori_color"].astype(np.float32)
        out["settings"] = np.array([model[k] for k in ("refl_msk_thr", "rough_msk_thr", "enlarge_scale")])
        uf = lambda k: torch.from_numpy(out[f"u_{k}"])
        # the condition on the inputs, over every call recorded below (the three sequences are made of these)
        margins = {"reset_opacity0": ms.reset_opacity0(model)[1], "reset_opacity1": ms.reset_opacity1(model, exclusive)[1],
                   "reset_refl": ms.reset_refl(model, exclusive)[1], "reset_refl 0.3": ms.reset_refl(model, exclusive, 0.3)[1],
                   "reset_refl 0.1": ms.reset_refl(model, exclusive, 0.1)[1], "reset_refl_strength2": ms.reset_refl_strength2(model)[1],
                   "dist_color": ms.dist_color(model, u["f_dc"], exclusive)[1], "dist_albedo": ms.dist_albedo(model, u["ori_color"], exclusive)[1],
                   "reset_scale": ms.reset_scale(model, exclusive)[1], "enlarge_refl_scales": ms.enlarge_refl_scales(model, False, exclusive)[1]}
        assert min(margins.values()) >= 1e-3, margins

        def run(key, call, reads, given=()):
            m = make(cls, model)
            before = {a: getattr(m, a) for a in GROUP_ATTRS.values()}
            _GIVEN_UNIFORMS[:] = [uf(k) for k in given]
            call(m)
            assert not _GIVEN_UNIFORMS
            for grp in reads:
                p = getattr(m, GROUP_ATTRS[grp])
                assert p is not before[GROUP_ATTRS[grp]], (key, grp)            # the method did replace the group
                st = m.optimizer.state[p]
                assert float(st["step"]) == 5.0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
                out[f"{key}__{grp}"] = p.detach().numpy().copy()

        run("reset_opacity0", lambda m: m.reset_opacity0(), ["opacity"])
        run("reset_opacity1", lambda m: m.reset_opacity1(), ["opacity"])
        run("reset_opacity1_excl", lambda m: m.reset_opacity1(exclusive_msk=excl), ["opacity"])
        run("reset_refl", lambda m: m.reset_refl(), ["refl_strength"])
        run("reset_refl_excl", lambda m: m.reset_refl(exclusive_msk=excl), ["refl_strength"])
        run("reset_refl_excl_030", lambda m: m.reset_refl(exclusive_msk=excl, rst_value=0.3), ["refl_strength"])
        run("reset_refl_strength", lambda m: m.reset_refl_strength(), ["refl_strength"])
        run("reset_refl_strength2", lambda m: m.reset_refl_strength2(), ["refl_strength"])
        run("reset_roughness", lambda m: m.reset_roughness(0.25), ["roughness"])
        run("reset_ori_color", lambda m: m.reset_ori_color(), ["ori_color"], ["ori_color"])
        run("reset_features", lambda m: m.reset_features(), ["f_dc", "f_rest"])
        run("dist_color", lambda m: m.dist_color(), ["f_dc"], ["f_dc"])
        run("dist_color_excl", lambda m: m.dist_color(exclusive_msk=excl), ["f_dc"], ["f_dc"])
        run("dist_albedo_excl", lambda m: m.dist_albedo(exclusive_msk=excl), ["ori_color"], ["ori_color"])
        run("reset_scale", lambda m: m.reset_scale(), ["scaling"])
        run("reset_scale_excl", lambda m: m.reset_scale(exclusive_msk=excl), ["scaling"])
        m = make(cls, model)
        out["enlarge_refl_scales_activated_excl"] = m.enlarge_refl_scales(ret_raw=False, exclusive_msk=excl).detach().numpy().copy()

        def normal_prop(m):                                                     # train_refnerf.py:1450-1455
            m.reset_opacity1(exclusive_msk=excl)
            m.dist_color(exclusive_msk=excl)
            m.reset_scale(exclusive_msk=excl)

        def opacity_reset(m):                                                   # :1439-1443
            m.reset_opacity0()
            m.reset_refl(exclusive_msk=excl, rst_value=0.1)

        def material_reset(m):                                                  # reset_gaussian_para2, :1524-1528
            m.reset_ori_color()
            m.reset_refl_strength(0.1)
            m.reset_roughness(0.2)
            m.reset_features()
        run("seq_normal_propagation", normal_prop, ["opacity", "f_dc", "scaling"], ["f_dc"])
        run("seq_opacity_reset", opacity_reset, ["opacity", "refl_strength"])
        run("seq_material_reset", material_reset, ["ori_color", "refl_strength", "roughness", "f_dc", "f_rest"], ["ori_color"])

        # ---- the two direction grids
        out["env_direction1_8x16"] = ns["get_env_direction1"](8, 16).numpy()
        out["env_direction2_8x16"] = ns["get_env_direction2"](8, 16).numpy()

        # ---- get_normal with the learned offsets
        g = torch.Generator().manual_seed(11)
        n = 16
        small = {k: torch.randn((n,) + s, generator=g).numpy().astype(np.float64) for k, s in
                 (("xyz", (3,)), ("rotation", (4,)), ("normal1", (3,)), ("normal2", (3,)))}
        small["scaling"] = torch.randn((n, 2), generator=g).numpy().astype(np.float64) * 0.3 - 1.0
        small["normal1"] *= 0.1
        small["normal2"] *= 0.1
        dirs = torch.nn.functional.normalize(torch.randn((n, 3), generator=g))
        full = dict(model, **small)
        for k in ms.GROUPS:
            if k != "scaling":
                full[k] = model[k][:n]
        m = make(cls, full, n)
        normals, delta = m.get_normal(1.0, dirs, return_delta=True)
        plain = m.get_normal(1.0, dirs)
        for k in ("xyz", "rotation", "normal1", "normal2", "scaling"):
            out[f"normal_in_{k}"] = small[k].astype(np.float32)
        out["normal_in_dirs"] = dirs.numpy()
        out["normal_out"], out["normal_out_delta"], out["normal_out_plain"] = normals.detach().numpy(), delta.detach().numpy(), plain.detach().numpy()
        assert 0 < int((delta.detach() == m._normal2.detach()).all(dim=1).sum()) < n          # both sides occur

        # ---- capture(): which attribute sits where
        m.active_sh_degree, m.spatial_lr_scale = 7, 3.25
        m.max_radii2D, m.xyz_gradient_accum, m.denom = torch.zeros(n), torch.zeros(n, 1), torch.zeros(n, 1)
        names = []
        for entry in m.capture():
            if isinstance(entry, dict):
                names.append("optimizer.state_dict()")
            elif isinstance(entry, torch.Tensor):
                names.append(next(k for k, v in vars(m).items() if v is entry))
            else:
                names.append({7: "active_sh_degree", 3.25: "spatial_lr_scale"}[entry])
        out["capture_order"] = np.array(names)
    path = os.path.join(HERE, "reference_model.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
